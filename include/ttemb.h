/*
 * ttemb.h -- C ABI of libttemb_hip.so: the MI355X (gfx950) Tensor-Train embedding
 * hot path.
 *
 * Every entry point replaces one function of the reference's pybind module
 * `tt_embeddings` (FBTT/tt_embeddings.cpp:131-161); the replaced interface is cited
 * per function.  The boundary is plain C: raw device pointers, explicit sizes, an
 * opaque `hipStream_t` passed as `void*`, a caller-provided workspace.  No allocation,
 * no host synchronisation unless a function says so, and no state in the library between
 * calls except process-wide DIAGNOSTIC switches that never change a result: the kernel-family
 * override (ttemb_set_path), the piece limits (ttemb_set_piece_limits), the spin limit (ttemb_set_spin_limit) and the
 * event profiler (ttemb_profile_enable) -- and one pinned host word through which a device-side wait that ran out is
 * reported (ttemb_init / ttemb_status).  A caller that never touches them has none.
 *
 * Tracing: with TTEMB_ROCTX=1 in the environment every lookup / cache entry point is bracketed by a roctx range
 * (roctxRangePush / Pop from librocprofiler-sdk-roctx.so or libroctx64.so, looked up at run time), so a
 * `rocprofv3 --marker-trace --kernel-trace` timeline shows the calls above their kernels.
 *
 * The workspace: every op leaves the first 40 KB of its workspace alone except the grouped
 * lookup, which keeps a call counter and a few pre-tagged counters there (in DEVICE memory, so
 * that a replayed HIP graph counts on).  Whatever those bytes hold is valid -- a fresh or
 * recycled buffer costs the first call a slower counting step, never a wrong result -- so
 * nothing has to be initialised; handing the same workspace to successive calls (what the
 * Python class does) keeps the fast step.  One workspace must not serve two streams at once.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - cores[t] is float32 [p_t][R_t*q_t*R_{t+1}] row-major, a core row being a
 *     row-major [R_t][q_t][R_{t+1}] block (FBTT/tt_embeddings_ops.py:528-545);
 *   - ids are int64, decomposed with L = [p1*p2.., .., 1] by repeated div/mod
 *     (FBTT/tt_embeddings_cuda.cu:796-802);
 *   - `rowidx[n]` is the bag (output row) of position n, non-decreasing inside the
 *     TT part and inside the cached part (what preprocess produces).  Where a function
 *     takes both `rowidx` and `offsets`, rowidx may be NULL when offsets (int64[B+1]) is
 *     given and the ids are exactly the concatenated bags: the rows are then derived
 *     from offsets inside the call (no separate ttemb_preprocess launch needed);
 *   - return value: 0 = ok, <0 = error (TTEMB_E_*), text via ttemb_last_error().
 */
#ifndef TTEMB_H_
#define TTEMB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTEMB_ABI_VERSION 4   /* 4: + the *_window calls (one table of a table-batched call); 3: + ttemb_init / ttemb_status / ttemb_set_spin_limit, TTEMB_FAMILY_PREFIX_IN_CHAIN, plan of G + 3 group words */
#define TTEMB_MAX_CORES 4

enum {
  TTEMB_OK = 0,
  TTEMB_E_BADARG = -1,     /* shape / size / null-pointer check failed            */
  TTEMB_E_WORKSPACE = -2,  /* workspace too small (see ttemb_workspace_bytes)      */
  TTEMB_E_UNSUPPORTED = -3,/* shape outside what the kernels support               */
  TTEMB_E_HIP = -4         /* a HIP runtime call failed (message has the detail)   */
};

/* TT factorisation of one table.  R has T+1 entries with R[0] = R[T] = 1. */
typedef struct ttemb_shape {
  int32_t T;                    /* number of cores, 2..4                          */
  int32_t p[TTEMB_MAX_CORES];   /* row factors,    prod(p) >= num_embeddings       */
  int32_t q[TTEMB_MAX_CORES];   /* column factors, prod(q) == D, D % 4 == 0        */
  int32_t R[TTEMB_MAX_CORES + 1];
} ttemb_shape_t;

/* Which computation a workspace is being sized for. */
enum {
  TTEMB_OP_FORWARD = 0,
  TTEMB_OP_BACKWARD = 1,        /* dense / sgd / adagrad all use the same size    */
  TTEMB_OP_PREPROCESS = 2,
  TTEMB_OP_CACHE_POPULATE = 3   /* nnz = hashtbl_size, B = cache rows              */
};

/* Kernel-selection knob for forward/backward (tests drive both; 0 is the default). */
enum {
  TTEMB_PATH_AUTO = 0,          /* grouped MFMA path when the shape has it and the batch is past its measured crossover
                                   (max(4096, p0*p1/4) ids; ranks >= 64: p0*p1/8 at 64, p0*p1/24 at 128, any at 256), else the
                                   per-bag MFMA kernels (ids + offsets), else generic */
  TTEMB_PATH_GENERIC = 1,       /* shape-generic wave-per-id kernels (T = 2..4)    */
  TTEMB_PATH_FAST3 = 2,         /* sorted / grouped MFMA path at every batch size, wherever the table has it (3 cores, or a
                                   2- / 4-core table on its 3-core view; inside the table-size limits of DESIGN.md 6c); else generic,
                                   as ttemb_kernel_family answers */
  TTEMB_PATH_PER_BAG = 3        /* one wavefront per bag (MFMA per id) whenever the shape has it and the ids come
                                   with their offsets, at every batch size; else generic.  For crossover measurements */
};

int ttemb_abi_version(void);
const char* ttemb_last_error(void);   /* thread-local, valid until the next call  */

/* Bytes of scratch the op needs for `nnz` ids and `B` bags (0 is a valid answer). */
int64_t ttemb_workspace_bytes(const ttemb_shape_t* shape, int32_t op, int64_t nnz, int64_t B);

/* Bytes of an id-grouping plan for `nnz` ids (0 when the selected kernel family needs none).
 * ttemb_forward leaves its grouping of the ids in a caller buffer of this size; passing the same
 * buffer to the backward of the SAME (indices, rowidx, nnz, nnz_dev) skips the regrouping.  The plan also
 * carries the prefix products G0[i0].G1[i1] the forward used: a backward handed the plan differentiates the
 * chain at those (the saved-tensor meaning of autograd); one that is not forms them from the cores it is given. */
int64_t ttemb_plan_bytes(const ttemb_shape_t* shape, int64_t nnz);

/* Select the kernel family used by later calls, process-wide (TTEMB_PATH_*). */
int ttemb_set_path(int32_t path);

/* A call whose [B][D] tensor does not fit one 32-bit window of byte offsets (2^24 rows or 2 GiB: what the grouped kernels
 * address through buffer descriptors) -- SAGE.inference looks up every node of the graph in one call, gnn_model.py:220-253 --
 * runs on the grouped path as a sequence of PIECES of the id list (the reference chunks any call by batch_count,
 * tt_embeddings_cuda.cu:1011-1027).  The boundaries follow `offsets` and are computed on the device: no host
 * synchronisation.  Needs `offsets`; ttemb_plan_bytes() is 0 for such a call (the backward regroups piece by piece), and
 * the fused backward entry points write the summed gradient into the workspace and step once.
 * DIAGNOSTIC, process-wide: smaller limits than the hardware's (rows per piece, ids per piece; 0 = default), so that
 * tests can cut a small call into many pieces.  Never changes a result. */
int ttemb_set_piece_limits(int64_t rows, int64_t ids);

/* DIAGNOSTIC, process-wide: the number of ids from which the backward of the wide-rank chain (ranks 64 / 128 / 256) reduces
 * dG2 inside its chunk kernel (LDS slabs, no E table) instead of writing one E row per id and reducing them in a second
 * kernel.  0 = the library's rule (8 ids per slab row: the slabs are written whatever the batch), 1 = always, a huge value =
 * never.  Changes workspace sizes (ask ttemb_workspace_bytes again); never changes a result beyond fp32 summation order. */
int ttemb_set_wide_slab_min_ids(int64_t ids);

/* Device-side faults.  The grouping pass of the grouped lookup has two BOUNDED waits between workgroups (the take-over of a
 * range counter that carries another call's tag, and the place step's look back at the chunk totals of the ranges before
 * it).  They cannot run out on a GPU that runs the launch's workgroups together; under CU masking, profiler
 * serialisation or several processes time-sliced on one GPU they can.  A wait that runs out never becomes plausible
 * numbers (the reference's kernels cannot time out; it checks its launches with AT_CUDA_CHECK,
 * FBTT/tt_embeddings_cuda.cu:1666,1742,1845):
 *   - the call's plan is POISONED on the device: the forward writes NaN into its whole output window, a backward on that
 *     plan writes NaN gradients; no kernel walks the chunk table.  A FUSED backward (ttemb_backward_sgd / _adagrad) on a
 *     poisoned plan leaves the parameters and the optimizer state UNTOUCHED when the host word below exists (the step can
 *     be repeated); without the word -- a graph captured before ttemb_init() -- it writes NaN parameters, the only signal
 *     such a graph has;
 *   - the reason is stored to a pinned host word, and the next ttemb_forward* / ttemb_backward* call of the process that
 *     sees it returns TTEMB_E_HIP with a message (once per fault, consumed by exactly one caller through an atomic
 *     exchange; no synchronisation is added for this).  The error refers to an EARLIER call; the call that returns it has
 *     not been started.
 * ttemb_init() creates that word (64 bytes of pinned, device-mapped host memory -- the ONE allocation this library ever
 * makes, which is why it is a call of its own and no lookup does it): call it once per process, from the host, OUTSIDE any
 * stream capture and before capturing a graph that contains grouped lookups.  Lookups made before it report an expired wait
 * through their NaN results only.  Idempotent; TTEMB_E_HIP when the memory cannot be had.
 * ttemb_status() is the check as a call of its own, for callers that synchronise: 0, or TTEMB_E_HIP (and the fault is
 * consumed); it creates the word when ttemb_init() has not.  ttemb_set_spin_limit is a DIAGNOSTIC, process-wide: tries of
 * those waits (0 = the default of 2^20, about 1.5 s; negative = none at all, every wait expires -- how tests reach the
 * fault path). */
int ttemb_init(void);
/* Byte offset, inside the header every lookup workspace begins with, of the uint32 the LAST grouped backward on that
 * workspace left: 1 = its plan was poisoned and the host word exists (gradients NaN, a fused update skipped), 0 = healthy.
 * Written by every backward of the grouped families (ttemb_kernel_family & 7 in {GROUPED, GROUPED_WIDE}); not written by the
 * others, which have no bounded waits. */
#define TTEMB_HEADER_POISON_OFFSET 32784
int ttemb_status(void);
int ttemb_set_spin_limit(int64_t tries);
/* DIAGNOSTIC (tests): the layout of the grouped path's id grouping pass for `nnz` ids on this table -- it launches nothing.
 * out[5] = {slices of the id list, ranges of the group space, banks of range counters, entries per (range, bank) bucket,
 * slots of the overflow area}.  TTEMB_E_UNSUPPORTED for a shape without grouped kernels. */
int ttemb_grouping_layout(const ttemb_shape_t* shape, int64_t nnz, int64_t* out);

/* Which kernels a lookup of `nnz` ids in `B` bags on this table would run, under the current ttemb_set_path: a
 * DIAGNOSTIC for tests, benchmarks and tuners (tuning_SAGE.py searches ranks in [2, 256]) -- it launches nothing.
 * `ids_with_offsets` != 0: the ids come with their bag boundaries and no row index (what TTEmbeddingBag.forward passes).
 *   TTEMB_FAMILY_SCALAR   wave-per-id kernels, plain FMA (any T, any shape)
 *   TTEMB_FAMILY_PER_BAG  one wavefront per bag, fp32 MFMA per id, an instantiated (q, ranks) shape
 *   TTEMB_FAMILY_PER_BAG_RT  the same with run-time (q, ranks): any 3-core shape with q0, q2 <= 16 and q0 q1 <= 64
 *   TTEMB_FAMILY_GROUPED  the grouped chain (ranks <= 32, an instantiated shape)
 *   TTEMB_FAMILY_GROUPED_WIDE  the grouped chain of ranks 64 / 128 / 256
 * | TTEMB_FAMILY_MERGED when a 2- or 4-core table rides on a 3-core view (a virtual core built per call),
 * | TTEMB_FAMILY_PADDED when a 3-core table whose ranks are off the instantiated list rides on the grouped kernels of the
 *   next listed rank through zero-padded copies of its cores (same rows, same gradients: the added rank positions hold
 *   zeros),
 * | TTEMB_FAMILY_PREFIX_IN_CHAIN when a whole ttemb_forward of this size forms the prefix products G0[i0].G1[i1] inside
 *   its chain kernel (fewer than 8 ids per (i0, i1) group on average, 16 for q0 = 8: 819 200 ids on the papers100M table) instead of in
 *   a launch of its own; the plan it leaves and every result are the same,
 * | TTEMB_FAMILY_GROUP_PRODUCTS_IN_CHAIN when a backward of this size forms the two per-group products (the dG0 parts and
 *   dG1: FBTT/tt_embeddings_cuda.cu:531-609 runs them as the t = 0 GEMM pair over a partial-product table) inside its chunk
 *   kernel, while a group's dP is still in registers: no dP table, no epilogue launch.  Same rule on the ids per group,
 *   for shapes whose dG2 reduction is not already fused into the chunk kernel (rank 32; large p2). */
enum {
  TTEMB_FAMILY_SCALAR = 0,
  TTEMB_FAMILY_PER_BAG = 1,
  TTEMB_FAMILY_PER_BAG_RT = 2,
  TTEMB_FAMILY_GROUPED = 3,
  TTEMB_FAMILY_GROUPED_WIDE = 4,
  TTEMB_FAMILY_MERGED = 16,
  TTEMB_FAMILY_PADDED = 32,
  TTEMB_FAMILY_PREFIX_IN_CHAIN = 64,
  TTEMB_FAMILY_GROUP_PRODUCTS_IN_CHAIN = 128
};
int ttemb_kernel_family(const ttemb_shape_t* shape, int64_t nnz, int64_t B, int32_t ids_with_offsets);

/* Measurement hook (bench.py's roofline leg).  While enabled (process-wide), the
 * main chain kernel of every ttemb_forward / ttemb_backward_* call is bracketed by
 * hipEvents on the call's stream.  ttemb_profile_read waits for the most recent bracket of
 * `which` (0 = forward chain kernel, 1 = all backward chain kernels, 2 = the backward chunk
 * kernel alone, 3 = the id-grouping pass including the prefix-product kernel, 4 = the cache probe pass of
 * ttemb_preprocess / ttemb_preprocess_update, 5 = its partition scatter, 6 = the cached-row gather of ttemb_cache_forward,
 * 7 = the cached-row update of ttemb_cache_backward_*, 8 = the group epilogue kernel of the backward, 9 = its finalize
 * kernel) and returns its duration in milliseconds; a slot no launch has bracketed since the last ttemb_profile_enable(1)
 * is TTEMB_E_BADARG (enabling forgets every earlier bracket).  Off by default; costs two event records per bracket when on. */
int ttemb_profile_enable(int32_t on);
int ttemb_profile_read(int32_t which, float* ms_host);

/* ---------------------------------------------------------------------------------
 * tt_forward  (replaces tt_embeddings.tt_forward -- FBTT/tt_embeddings.cpp:132,
 * tt_embeddings_forward_cuda FBTT/tt_embeddings_cuda.cu:967-1081).
 * output[B][D] is fully written: bag sums of the TT rows of indices[0:nnz], zeros
 * for bags with no id in that range.  `nnz_dev`, when non-null, points at a device
 * int32 holding the live count (<= nnz); the launch is sized by nnz and the kernels
 * read the count themselves, so no host sync is needed after ttemb_preprocess.
 * `offsets` (int64[B+1]) describes the bags of the ORIGINAL id list: with it only bags whose
 * length is not 1 are zero-filled before the lookups (a bag of one id has exactly one writer,
 * this call or ttemb_cache_forward(offsets)); with offsets == NULL the whole output is
 * zero-filled first and single-id detection falls back to neighbouring rowidx values.
 * `plan` (nullable, ttemb_plan_bytes() bytes) receives the id grouping (and the prefix products) for the backward.
 * plan == NULL is the INFERENCE form: the grouping lives and dies in the workspace, and a forward that forms its prefix
 * products inside the chain kernel (TTEMB_FAMILY_PREFIX_IN_CHAIN) stores none of them -- same rows, less HBM traffic.
 * There is no batch_count chunking: intermediates never leave the chip.
 * ------------------------------------------------------------------------------- */
int ttemb_forward(const ttemb_shape_t* shape, const float* const* cores,
                  const int64_t* indices, const int64_t* rowidx, const int64_t* offsets,
                  int64_t nnz, const int32_t* nnz_dev, int64_t B, float* output,
                  void* workspace, int64_t workspace_bytes, void* plan, int64_t plan_bytes,
                  void* stream);

/* Two-phase forward, for a caller that wants to overlap the id-only work with something that still writes the
 * cores (ttemb_dist.TTDataParallel: the all-reduce + update of the previous step):
 *   ttemb_forward_group   everything that depends only on the ids -- the grouping pass into `plan`, bag rows,
 *                         zeroing of the output rows of bags that do not hold exactly one id.  `cores` is not read.
 *   ttemb_forward_lookup  the rest: prefix products and the chain kernel, on the plan the first call filled.
 * Same arguments for both; `plan` (ttemb_plan_bytes() bytes) is required whenever ttemb_plan_bytes() != 0.
 * ttemb_forward == group followed by lookup.  When the selected kernel family keeps no plan, group does nothing
 * and lookup is the whole forward. */
int ttemb_forward_group(const ttemb_shape_t* shape, const float* const* cores,
                  const int64_t* indices, const int64_t* rowidx, const int64_t* offsets,
                  int64_t nnz, const int32_t* nnz_dev, int64_t B, float* output,
                  void* workspace, int64_t workspace_bytes, void* plan, int64_t plan_bytes,
                  void* stream);
int ttemb_forward_lookup(const ttemb_shape_t* shape, const float* const* cores,
                  const int64_t* indices, const int64_t* rowidx, const int64_t* offsets,
                  int64_t nnz, const int32_t* nnz_dev, int64_t B, float* output,
                  void* workspace, int64_t workspace_bytes, void* plan, int64_t plan_bytes,
                  void* stream);

/* ---------------------------------------------------------------------------------
 * tt_dense_backward  (tt_embeddings.tt_dense_backward -- tt_embeddings.cpp:133-136,
 * tt_embeddings_cuda.cu:656-686, 421-654).  d_cores[t] (same shape as cores[t]) is
 * overwritten with the gradient of sum(output * d_output) w.r.t. cores[t].
 * ------------------------------------------------------------------------------- */
int ttemb_backward_dense(const ttemb_shape_t* shape, const float* const* cores,
                         const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                         const int32_t* nnz_dev, int64_t B, const float* d_output,
                         float* const* d_cores,
                         void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes,
                         void* stream);

/* tt_sgd_backward (tt_embeddings.cpp:137-138, tt_embeddings_cuda.cu:688-719):
 * cores[t] -= lr * d_core_t, every row (the reference's grid defect at :633-651 is
 * not reproduced).  The gradient lives in the workspace only. */
int ttemb_backward_sgd(const ttemb_shape_t* shape, float* const* cores,
                       const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                       const int32_t* nnz_dev, int64_t B, const float* d_output, float lr,
                       void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes,
                       void* stream);

/* tt_adagrad_backward (tt_embeddings.cpp:139-142, tt_embeddings_cuda.cu:721-754,
 * 399-419): state += g*g ; core -= lr * g / (sqrt(state) + eps). */
int ttemb_backward_adagrad(const ttemb_shape_t* shape, float* const* cores,
                           float* const* opt_state,
                           const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                           const int32_t* nnz_dev, int64_t B, const float* d_output,
                           float lr, float eps,
                           void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------
 * A WINDOW of a longer id list: one table of a table-batched call.
 * Replaces, for `num_tables` > 1: the `tableidx` the reference's kernels derive per id (compute_rowidx_kernel,
 * tt_embeddings_cuda.cu:1349-1365) and index their per-table core pointers with (tt_embeddings_cuda.cu:443-609,
 * called by TableBatchedTTEmbeddingBag.forward, tt_embeddings_ops.py:862-916) -- the host never learns where a table's ids
 * begin.  Here a table is a call of its own on a window: the bags [bag0, bag0 + B) of `offsets` (int64[bags_total + 1], the
 * whole call's) and the ids that belong to them; where the window begins and ends in `indices` is read from `offsets` ON THE
 * DEVICE -- no host synchronisation.  `nnz` = length of the WHOLE id list (the launches are sized by it; a window that turns
 * out empty costs its launches and nothing else); `output` / `d_output` = the [bags_total][D] tensor of the whole call (the
 * window's rows are bag0 .. bag0 + B - 1; no other row is touched).  `cores` / `d_cores` / `opt_state` are the window's own
 * table.  Served by the grouped kernels, whatever the size: TTEMB_E_UNSUPPORTED (from the size query already) for a shape they
 * do not cover (2- / 4-core tables, ranks off the list) or a window past their limits -- the caller then splits the id list on
 * the host, one plain call per table.  Workspace: ttemb_window_workspace_bytes(shape, TTEMB_OP_FORWARD | TTEMB_OP_BACKWARD, ...);
 * one workspace serves every window and every other op.  A window keeps no plan: its backward groups the window's ids again.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_window_workspace_bytes(const ttemb_shape_t* shape, int32_t op, int64_t nnz, int64_t bags_total, int64_t B);
int ttemb_forward_window(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                         const int64_t* offsets, int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B,
                         float* output, void* workspace, int64_t workspace_bytes, void* stream);
int ttemb_backward_dense_window(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                                const int64_t* offsets, int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B,
                                const float* d_output, float* const* d_cores, void* workspace,
                                int64_t workspace_bytes, void* stream);
int ttemb_backward_sgd_window(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices,
                              const int64_t* offsets, int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B,
                              const float* d_output, float lr, void* workspace, int64_t workspace_bytes, void* stream);
int ttemb_backward_adagrad_window(const ttemb_shape_t* shape, float* const* cores, float* const* opt_state,
                                  const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t bags_total,
                                  int64_t bag0, int64_t B, const float* d_output, float lr, float eps,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Stage one call of ANY size into the static buffers of a captured lookup (no counterpart in the reference: it has no
 * graph capture).  A graph captured with nnz = nnz_cap, B = B_cap and nnz_dev = nnz_dev_out serves every call of
 * n_live <= nnz_cap ids in B_live <= B_cap bags once this ran in front of its replay.  ONE launch on `stream`, no host
 * synchronisation, no workspace.  `indices_in` holds n_live ids, int64 or (indices_are_i32 != 0) int32, widened here;
 * `offsets_in` the B_live + 1 bag boundaries, int64 or (offsets_are_i32 != 0) int32, or NULL: bags of one id, which needs
 * B_live == n_live.  Written:
 *     indices_out[0 : n_live]              the ids
 *     indices_out[n_live : nnz_cap]        NOT touched (ids that were valid earlier; no kernel reads past the count)
 *     offsets_out[0 : B_live + 1]          the offsets (0 .. B_live without offsets_in)
 *     offsets_out[B_live + 1 : B_cap + 1]  n_live: every bag past the live ones is empty
 *     *nnz_dev_out                         n_live
 * TTEMB_E_BADARG, with nothing launched, for a negative size, n_live > nnz_cap, B_live > B_cap, n_live or nnz_cap >= 2^31
 * (the count word is int32), a null output, null ids with n_live > 0, or offsets_in == NULL with B_live != n_live.
 * n_live == 0 is valid.  The inputs must not overlap the outputs.
 * ------------------------------------------------------------------------------- */
int ttemb_stage_call(const void* indices_in, int32_t indices_are_i32, int64_t n_live,
                     const void* offsets_in /* nullable */, int32_t offsets_are_i32, int64_t B_live,
                     int64_t* indices_out, int64_t nnz_cap,
                     int64_t* offsets_out, int64_t B_cap,
                     int32_t* nnz_dev_out, void* stream);

/* Flat optimiser epilogues over n floats (used after the data-parallel all-reduce of
 * the flattened core gradients; same arithmetic as tt_embeddings_cuda.cu:381-419). */
int ttemb_sgd_step(float* weights, const float* grads, int64_t n, float lr, void* stream);
/* The same step, skipped as a whole when the 32-bit device word *skip is non-zero (tested bit-wise: a float count k.0f and
 * the uint32 poison word of a workspace header both work; a single process passes the header word itself).  The data-parallel step (no counterpart in the
 * reference: its DDP path is a stub, sage_dgl_partition.py:198-255) all-reduces, next to the gradients, the number of ranks
 * whose gradient came from a POISONED plan (the word at TTEMB_HEADER_POISON_OFFSET of the workspace the backward ran on,
 * see "Device-side faults"): when any did, the summed gradient is NaN and every rank skips the update together -- replicas
 * stay identical and untouched, the faulted rank's next call returns TTEMB_E_HIP. */
int ttemb_sgd_step_guarded(float* weights, const float* grads, int64_t n, float lr, const float* skip, void* stream);
int ttemb_adagrad_step(float* weights, float* state, const float* grads, int64_t n,
                       float lr, float eps, void* stream);

/* ---------------------------------------------------------------------------------
 * Fused Adam / AdamW (no counterpart in the reference: its OptimType.ADAM dispatches to Adagrad, tt_embeddings_ops.py:229-286;
 * its drivers step the cores with torch.optim.Adam / AdamW).  DENSE Adam, as torch.optim.Adam(amsgrad=False) on the dense
 * core gradients: every element of every core moves on every applied step, also rows no id of the call touches (their g is
 * 0, their first moment is not).  Per element, t = the number of steps applied including this one:
 *     g' = g + wd w  (decoupled = 0)   |   w = w - lr wd w  (decoupled = 1, AdamW; g' = g)
 *     m = b1 m + (1 - b1) g' ;  v = b2 v + (1 - b2) g'^2 ;  w = w - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * (a zero denominator -- v = 0 and eps = 0 -- leaves w alone).  `exp_avg[t]` / `exp_avg_sq[t]`: m and v, shaped like cores[t].
 * `step`: int32[4] on the device, owned by the caller, all zero before the first step: word 0 is t; words 1-3 are scratch
 * of the call (t + 1 and the two bias corrections as float bits, formed on the device by one lane of a kernel of the same
 * call).  t lives on the device so that a captured graph and a deferred data-parallel step carry no host state; it advances
 * once per applied step.  A call without ids (nnz = 0) is a no-op and does not advance t.  A step that is SKIPPED (a grouped
 * call on a poisoned plan whose fault the host hears of, see "Device-side faults"; the `skip` word of ttemb_adam_step) leaves
 * w, m, v and t as they were.  On the grouped route of a one-piece call the step rides in the last backward kernel (no
 * launch added); every other route writes the gradient into the workspace and steps all cores in one launch behind a
 * one-lane launch that forms the pending step words.
 * ------------------------------------------------------------------------------- */
typedef struct ttemb_adam {
  float lr, eps, weight_decay;
  int32_t decoupled;      /* 0: torch.optim.Adam's coupled decay, 1: AdamW's */
  double beta1, beta2;    /* in [0, 1); double: the bias corrections are formed from them */
} ttemb_adam_t;
int ttemb_backward_adam(const ttemb_shape_t* shape, float* const* cores, float* const* exp_avg, float* const* exp_avg_sq,
                        int32_t* step, const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                        const int32_t* nnz_dev, int64_t B, const float* d_output, const ttemb_adam_t* hp,
                        void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes, void* stream);
/* one table of a table-batched call (see "A WINDOW of a longer id list"); `step` is that table's.  A window that turns out
 * empty on the device is a step on a zero gradient (m and v decay, t advances), what torch.optim.Adam does with it. */
int ttemb_backward_adam_window(const ttemb_shape_t* shape, float* const* cores, float* const* exp_avg, float* const* exp_avg_sq,
                               int32_t* step, const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t bags_total,
                               int64_t bag0, int64_t B, const float* d_output, const ttemb_adam_t* hp, void* workspace,
                               int64_t workspace_bytes, void* stream);
/* Flat epilogue over n floats (the data-parallel step): g = grads[i] * grad_scale (1 / world: the averaged gradient enters
 * m and v), then the step above.  `skip`: null, or a 32-bit device word tested bit-wise as in ttemb_sgd_step_guarded:
 * non-zero leaves weights, exp_avg, exp_avg_sq and step[0] untouched.  Buffers 16-byte aligned. */
int ttemb_adam_step(float* weights, float* exp_avg, float* exp_avg_sq, int32_t* step, const float* grads, int64_t n,
                    float grad_scale, const ttemb_adam_t* hp, const float* skip, void* stream);

/* ---------------------------------------------------------------------------------
 * Device-resident learning rate (no counterpart in the reference: it has no graph capture; torch.optim's
 * capturable=True with a tensor lr is the same idea).  Every call above takes the rate BY VALUE, so a captured backward
 * bakes it in.  The calls below take it as `lr_dev`: a DEVICE pointer to one float32 in 16-byte-aligned memory the caller
 * owns.  Every kernel that applies a step reads the word once, at its top, and then runs the arithmetic of its by-value
 * twin unchanged -- same value in the word, same bits out wherever the twin is deterministic.  No kernel writes the word.
 * A captured graph holds its ADDRESS: the rate of a replay is what the word holds when the replay runs, so a scheduler
 * changes it with one device-side write on the same stream and nothing is re-captured.  The value is NOT range-checked
 * (the host never sees it): a negative or NaN rate does what the arithmetic does.
 * `ttemb_step_t` describes the step:
 *     kind       TTEMB_STEP_SGD | TTEMB_STEP_ADAGRAD | TTEMB_STEP_ADAM
 *     lr_dev     the word; NULL or misaligned is TTEMB_E_BADARG with nothing launched
 *     eps        Adagrad's (Adam's is adam->eps; SGD ignores it)
 *     state      per core, like `cores`: the Adagrad state / Adam's exp_avg (SGD: ignored)
 *     state2     per core: Adam's exp_avg_sq (else ignored)
 *     adam_step  Adam's int32[4] device words (see "Fused Adam / AdamW"; else ignored)
 *     adam       Adam's hyper-parameters; its `lr` is IGNORED (else the pointer is ignored)
 * The four calls mirror ttemb_backward_sgd / _adagrad / _adam, their *_window and *_exact forms and the flat epilogues,
 * argument for argument, with the optimiser arguments replaced by the descriptor; routes, workspace, plan, poisoned plans,
 * the nnz = 0 no-op and every other rule are those of the mirrored call.  ttemb_flat_step takes its arrays as arguments (the
 * descriptor's state / state2 / adam_step are not looked at): SGD (state, state2, adam_step NULL; `skip` as in
 * ttemb_sgd_step_guarded, or NULL), Adagrad (state; `skip` must be NULL) or Adam (state = exp_avg, state2 = exp_avg_sq,
 * adam_step; `skip` as in ttemb_adam_step); `grad_scale` is Adam's and must be 1 for the other two.
 * ------------------------------------------------------------------------------- */
enum { TTEMB_STEP_SGD = 0, TTEMB_STEP_ADAGRAD = 1, TTEMB_STEP_ADAM = 2 };
typedef struct ttemb_step {
  int32_t kind;
  const float* lr_dev;
  float eps;
  float* const* state;
  float* const* state2;
  int32_t* adam_step;
  const ttemb_adam_t* adam;
} ttemb_step_t;
int ttemb_backward_step(const ttemb_shape_t* shape, float* const* cores,
                        const int64_t* indices, const int64_t* rowidx, const int64_t* offsets, int64_t nnz,
                        const int32_t* nnz_dev, int64_t B, const float* d_output, const ttemb_step_t* step,
                        void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes,
                        void* stream);
/* one table of a table-batched call (see "A WINDOW of a longer id list"); step->adam_step is that table's */
int ttemb_backward_step_window(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices,
                               const int64_t* offsets, int64_t nnz, int64_t bags_total, int64_t bag0, int64_t B,
                               const float* d_output, const ttemb_step_t* step, void* workspace,
                               int64_t workspace_bytes, void* stream);
/* exact mode (see "Exact mode"): the results are a function of the inputs and of the VALUE in the word, bit for bit */
int ttemb_backward_step_exact(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices,
                              const int64_t* offsets, int64_t nnz, int64_t B, const float* d_output,
                              const ttemb_step_t* step, void* workspace, int64_t workspace_bytes,
                              const void* plan, int64_t plan_bytes, void* stream);
int ttemb_flat_step(float* weights, float* state, float* state2, int32_t* adam_step, const float* grads, int64_t n,
                    float grad_scale, const ttemb_step_t* step, const float* skip, void* stream);

/* ---------------------------------------------------------------------------------
 * LFU hash-table cache.
 * update_cache_state (tt_embeddings.cpp:144, tt_embeddings_cuda.cu:1083-1119):
 * insert every id with count+1 (Murmur3-style hash, <=3 linear probes, 64-bit CAS;
 * hashtbl_cuda_utils.cuh:48-133).  hashtbl/cache_freq are int64[H].
 * ------------------------------------------------------------------------------- */
int ttemb_cache_update(const int64_t* indices, int64_t nnz, int64_t* hashtbl,
                       int64_t* cache_freq, int64_t H, void* stream);

/* The same update with the reference's ONE-SWEEP insert (hashtbl_cuda_utils.cuh:102-133: the first probe slot that is
 * empty or holds the key takes the count), for callers that need the reference's table bit for bit.  ttemb_cache_update
 * looks the key up in all of its probe slots first: identical tables until cache_populate has evicted keys; afterwards
 * the one-sweep form can re-insert a cached id into a hole in front of its slot, after which the id resolves to the new
 * slot and drops out of the cache (which ids depends on thread order). */
int ttemb_cache_update_one_sweep(const int64_t* indices, int64_t nnz, int64_t* hashtbl, int64_t* cache_freq,
                                 int64_t H, void* stream);

/* cache_populate (tt_embeddings.cpp:145, tt_embeddings_cuda.cu:1270-1347): stable
 * descending sort of the H slots by frequency, keep ranks < C (cache_state[slot] =
 * rank), evict the rest, fill cache_weight[C][D] with the TT rows of the kept ids
 * (empty ranks stand for id 0, as in the reference). */
int ttemb_cache_populate(const ttemb_shape_t* shape, const float* const* cores,
                         int64_t* hashtbl, int64_t* cache_freq, int32_t* cache_state,
                         int64_t H, float* cache_weight, int64_t C,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* preprocess_indices_sync (tt_embeddings.cpp:146-149, tt_embeddings_cuda.cu:1388-1507),
 * single table.  Always writes rowidx_out[nnz] from offsets[B+1].  With warmup != 0
 * (or H == 0) indices are passed through (indices_out may alias indices or be null) and
 * *nnz_tt_dev = nnz.  Otherwise ids are looked up in the cache and (indices, rowidx,
 * cache_loc) are partitioned: TT ids first in input order, cached ids from the end
 * backwards (the CUB DevicePartition::Flagged order); *nnz_tt_dev = #TT ids.
 * Does NOT synchronise: the count stays on the device (pass it to the other entry
 * points as nnz_dev, or copy it back yourself).
 * `dup_stamp` (nullable; int32[C] of scratch, any content) turns on duplicate detection among the cached ids:
 * nnz_tt_dev must then hold TWO int32 and nnz_tt_dev[1] becomes 1 when some cache row is met more than once in
 * this call, else 0 -- the word ttemb_cache_backward_sgd / _dense take as `dup_dev`.  (Every cached id stamps its
 * row with its position, the partition step reads the stamps back.)  `epoch` is ignored (ABI 1 needed it). */
int ttemb_preprocess(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                     int32_t warmup, const int64_t* hashtbl, const int32_t* cache_state,
                     int64_t H, int64_t* indices_out, int64_t* rowidx_out,
                     int32_t* cache_loc_out, int32_t* nnz_tt_dev, int32_t* dup_stamp, int32_t epoch,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* update_cache_state + preprocess_indices_sync in ONE probe pass -- what TTEmbeddingBag.forward does with a live cache
 * (tt_embeddings_ops.py:836-870 calls the two back to back on the same ids, and both visit the same <= 3 slots per id).
 * Same hashtbl / cache_freq / outputs as ttemb_cache_update followed by ttemb_preprocess(warmup = 0): the find-first
 * update never moves or evicts a key, so an id resolves to the same slot before and after its batch was counted.
 * (A caller that needs the reference's one-sweep insert keeps the two calls apart.) */
int ttemb_preprocess_update(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                            int64_t* hashtbl, int64_t* cache_freq, const int32_t* cache_state, int64_t H,
                            int64_t* indices_out, int64_t* rowidx_out, int32_t* cache_loc_out,
                            int32_t* nnz_tt_dev, int32_t* dup_stamp, void* workspace, int64_t workspace_bytes,
                            void* stream);

/* cache_forward (tt_embeddings.cpp:151, tt_embeddings_cuda.cu:1509-1583):
 * output[rowidx[n]] += cache_weight[cache_loc[n]] for n in [start, nnz).  `start` is
 * the host value, or *start_dev when start_dev is non-null.  With `offsets` (the same
 * int64[B+1] given to ttemb_forward) a bag of exactly one id is written with a plain
 * store -- ttemb_forward(offsets) left such rows untouched, so nothing is read or zeroed. */
int ttemb_cache_forward(const int32_t* cache_loc, const int64_t* rowidx, const int64_t* offsets, int64_t start,
                        const int32_t* start_dev, int64_t nnz, const float* cache_weight,
                        int64_t D, float* output, void* stream);

/* cache_backward_sgd (tt_embeddings.cpp:152, tt_embeddings_cuda.cu:1585-1668):
 * cache_weight[loc] -= lr * d_output[row].  The adds are float atomics (an id may occur twice, as in the
 * reference) unless `dup_dev` (nullable) points at a device int32 that is 0: the word ttemb_preprocess wrote
 * when no cache row occurs twice in the call -- every row then has one writer and is updated by a plain
 * read-modify-write. */
int ttemb_cache_backward_sgd(const int32_t* cache_loc, const int64_t* rowidx, int64_t start,
                             const int32_t* start_dev, int64_t nnz, const float* d_output,
                             int64_t D, float lr, float* cache_weight, const int32_t* dup_dev, void* stream);

/* cache_backward_dense (tt_embeddings.cpp:153-156, tt_embeddings_cuda.cu:1670-1744):
 * d_cache_weight[C][D] is zero-filled, then d_cache_weight[loc] += d_output[row]. */
int ttemb_cache_backward_dense(const int32_t* cache_loc, const int64_t* rowidx, int64_t start,
                               const int32_t* start_dev, int64_t nnz, const float* d_output,
                               int64_t D, int64_t C, float* d_cache_weight, const int32_t* dup_dev, void* stream);

/* cache_backward_rowwise_adagrad_approx (tt_embeddings.cpp:157-160,
 * tt_embeddings_cuda.cu:1746-1846): per id, g2 = mean(d_output[row]^2);
 * old = atomic_add(state[loc], g2); cache_weight[loc] -= lr/(sqrt(old+g2)+eps) * d_output[row]. */
int ttemb_cache_backward_rowwise_adagrad(const int32_t* cache_loc, const int64_t* rowidx,
                                         int64_t start, const int32_t* start_dev, int64_t nnz,
                                         const float* d_output, int64_t D, float lr, float eps,
                                         float* cache_state_sum, float* cache_weight,
                                         void* stream);

/* ---------------------------------------------------------------------------------
 * Exact mode (OptimType.EXACT_SGD, FBTT/tt_embeddings_ops.py: "deterministic updates (via sorting + segment
 * reduction)").  A kernel family of its own (ttemb_exact.hip): the outputs, gradients, updated cores and optimizer state
 * are a function of (shape, cores, indices, offsets, B, d_output, lr, eps) only, bit for bit.  Nothing that sets a
 * floating-point summation order depends on the grid size or the number of CUs, on workgroup scheduling or other work on
 * the GPU, on the previous contents of the workspace, or on whether the call is eager or replayed from a captured graph:
 *   - no float atomics; the only atomics are the integer digit counts of the sort, whose order sets nothing;
 *   - no waits between workgroups (no look-back, no spin): nothing can expire, there is no poisoned plan to report;
 *   - every loop over work items is grid-stride, and every chunk boundary comes from the sorted id list alone;
 *   - no host synchronisation and no allocation (like every other lookup: an exact call can be captured).
 * Forward: one wave per bag sums its ids' rows in position order and stores the bag row once (empty bags: zeros).
 * Backward: the positions are sorted by i0, by i1 and by i2 (stable LSD radix sort: positions in order inside a row);
 * each core row sums its ids' contributions in that order, in fixed chunks of the sorted list whose partials are added in
 * chunk order.  Dense: every row of d_cores is written (untouched rows 0).  SGD / Adagrad: only the rows some id touches
 * are updated; every other row and its optimizer state stay bitwise unchanged.
 * Domain: 3-core views with q0, q2 <= 16, q0 q1 <= 64 and ranks <= 32 (any rank in that range, no padding).  A 2-core
 * table runs with an identity middle core.  A 4-core table merges one adjacent pair into a virtual core (workspace; each
 * element a sum in a fixed order), the pair chosen as the one whose view fits with the smallest virtual core, and its
 * gradient is split back into the pair's gradients in a fixed order.  TTEMB_E_UNSUPPORTED with a message for everything
 * else (ranks 64..256, larger q, a 4-core table none of whose pairs gives such a view) and for a call without `offsets`
 * (int64[B+1], required; the ids are the concatenated bags).  A live LFU cache is the caller's to exclude: these calls
 * never look at one.
 * Workspace: ttemb_exact_workspace_bytes() serves the forward and every backward; only a 4-core table's forward uses it.
 * `plan` / `plan_bytes` are reserved: ttemb_exact_plan_bytes() is 0 today and the calls ignore the two arguments (pass
 * NULL, 0).  The backward sorts the ids itself and forms every product from the cores it is given; a later version may
 * keep the sort and the group products there, sized by ttemb_exact_plan_bytes(), without changing these signatures.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_exact_workspace_bytes(const ttemb_shape_t* shape, int64_t nnz, int64_t B);   /* forward and backward */
int64_t ttemb_exact_plan_bytes(const ttemb_shape_t* shape, int64_t nnz);
/* DIAGNOSTIC, process-wide: caps the grid of every exact kernel at `workgroups` (0 = the default).  Under the contract it
 * never changes a result; tests use it to show that. */
int ttemb_set_exact_grid(int32_t workgroups);
int ttemb_forward_exact(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                        const int64_t* offsets, int64_t nnz, int64_t B, float* output,
                        void* workspace, int64_t workspace_bytes, void* plan, int64_t plan_bytes, void* stream);
int ttemb_backward_dense_exact(const ttemb_shape_t* shape, const float* const* cores, const int64_t* indices,
                               const int64_t* offsets, int64_t nnz, int64_t B, const float* d_output,
                               float* const* d_cores, void* workspace, int64_t workspace_bytes,
                               const void* plan, int64_t plan_bytes, void* stream);
int ttemb_backward_sgd_exact(const ttemb_shape_t* shape, float* const* cores, const int64_t* indices,
                             const int64_t* offsets, int64_t nnz, int64_t B, const float* d_output, float lr,
                             void* workspace, int64_t workspace_bytes, const void* plan, int64_t plan_bytes, void* stream);
int ttemb_backward_adagrad_exact(const ttemb_shape_t* shape, float* const* cores, float* const* opt_state,
                                 const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                                 const float* d_output, float lr, float eps, void* workspace, int64_t workspace_bytes,
                                 const void* plan, int64_t plan_bytes, void* stream);
/* Adam in exact mode (see "Fused Adam / AdamW"): ttemb_backward_dense_exact into scratch, then the flat step core by core --
 * an elementwise step has no order, so cores, exp_avg and exp_avg_sq are a function of the inputs only.  Unlike the exact
 * SGD / Adagrad steps it moves EVERY row (dense Adam).  Workspace: ttemb_exact_workspace_bytes() PLUS, behind it, the
 * gradient scratch: the sum over the table's cores of their bytes, each rounded up to 256. */
int ttemb_backward_adam_exact(const ttemb_shape_t* shape, float* const* cores, float* const* exp_avg, float* const* exp_avg_sq,
                              int32_t* step, const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B,
                              const float* d_output, const ttemb_adam_t* hp, void* workspace, int64_t workspace_bytes,
                              const void* plan, int64_t plan_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Weighted and mean bags (torch.nn.functional.embedding_bag with include_last_offset=True: mode "sum" with
 * per_sample_weights, and mode "mean").  These calls pool rows the lookups produced; they never read a core (ttemb_bag.hip).
 *   - weighted sum: look the ids up as nnz bags of one (offsets = 0, 1, ..., nnz), then
 *     ttemb_bag_reduce: output[b] = sum_{i in bag b} weights[i] rows[i], ids in position order; the backward
 *     ttemb_bag_reduce_backward writes d_rows[i] = weights[i] d_output[bag(i)] (which any lookup backward then takes with
 *     the same bags of one) and, when d_weights is not NULL, d_weights[i] = <d_output[bag(i)], rows[i]>;
 *   - mean: the plain lookup with the real offsets, then ttemb_bag_mean: dst[b] = src[b] / len(b) (a division; dst may
 *     alias src); the backward is ttemb_bag_mean on d_output into scratch, then the plain lookup backward.
 * rows / d_rows are float32 [nnz][D], output / d_output / src / dst [B][D], weights / d_weights float32 [nnz], offsets
 * int64 [B + 1] over the concatenated bags.  D is a positive multiple of 4 and the [.][D] buffers are 16-byte aligned.
 * An empty bag gives zeros; an id outside every bag gets zero d_rows / d_weights.
 * Deterministic by construction, as exact mode: no float atomics, no waits between workgroups, grid-stride loops whose
 * grid is capped by ttemb_set_exact_grid, summation orders set by `offsets` and D alone.  A bag of more than 512 ids is
 * summed in the fixed chunks [512 k, 512 (k + 1)) of the position list, whose partials (workspace) are added in chunk order.
 * ttemb_bag_workspace_bytes sizes the workspace of ttemb_bag_reduce; it lies behind the 40 KB header, so the workspace of
 * the lookups serves these calls too.  ttemb_bag_reduce_backward does not use its workspace today (pass the same one).
 * No host synchronisation and no allocation.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_bag_workspace_bytes(int64_t nnz, int64_t B, int64_t D);
int ttemb_bag_reduce(const float* rows, const float* weights, const int64_t* offsets, int64_t nnz, int64_t B, int64_t D,
                     float* output, void* workspace, int64_t workspace_bytes, void* stream);
int ttemb_bag_reduce_backward(const float* d_output, const float* weights, const float* rows /* NULL: no d_weights */,
                              const int64_t* offsets, int64_t nnz, int64_t B, int64_t D, float* d_rows,
                              float* d_weights /* NULL: no weight gradient */, void* workspace, int64_t workspace_bytes,
                              void* stream);
int ttemb_bag_mean(const float* src, float* dst, const int64_t* offsets, int64_t B, int64_t D, void* stream);

/* ---------------------------------------------------------------------------------
 * Max bags (torch.nn.functional.embedding_bag's mode "max", include_last_offset=True).  As the weighted sum: look the ids
 * up as nnz bags of one, then pool the rows here; no core is read (ttemb_bag.hip).
 *   - ttemb_bag_max: output[b][d] = max over the kept positions i of bag b of rows[i][d], and argmax[b][d] (int32) = the
 *     FIRST position of this call's id list that holds it: walking the bag in position order a later position wins only
 *     with a strictly larger value, so of equal values (+0.0 and -0.0 are equal) the earlier position stays.  NaN is never
 *     swallowed: a NaN in any kept position makes the element NaN and the winner is the first NaN position
 *     (take = v > best || (v != v && best == best)); torch's CPU kernel keeps a NaN only when it comes first.  A bag
 *     without a kept position (empty, or pads only) gives zeros and argmax -1.  `indices` (nullable): when given, a
 *     position whose raw id indices[i] equals `pad` is not kept (embedding_bag's padding_idx); NULL keeps every position
 *     and `pad` is ignored.
 *   - ttemb_bag_max_backward: d_rows[i][d] = d_output[bag(i)][d] where argmax[bag(i)][d] == i, else 0.  EVERY element of
 *     d_rows[nnz][D] is written -- zeros for pads and for positions outside every bag -- so no zero-fill pass is needed, and
 *     any lookup backward then takes d_rows with the same bags of one.
 * rows / d_rows are float32 [nnz][D], output / d_output float32 [B][D], argmax int32 [B][D], offsets int64 [B + 1] over the
 * concatenated bags.  D is a positive multiple of 4, the [.][D] buffers are 16-byte aligned, nnz < 2^31 (the positions are
 * int32); checks and error codes as the sum calls.  Deterministic by construction, as exact mode: no float atomics, no
 * waits between workgroups, grid-stride loops whose grid is capped by ttemb_set_exact_grid.  A bag of more than 512 ids is
 * cut into the fixed chunks [512 k, 512 (k + 1)) of the position list; their partial (value, position) pairs (workspace)
 * are combined in chunk order by the same strict rule, so the first position still wins.  Every workspace word that is read
 * was written earlier in the same call.  ttemb_bag_max_workspace_bytes sizes the workspace of ttemb_bag_max; it lies behind
 * the 40 KB header, so the workspace of the lookups serves it too.  No host synchronisation and no allocation.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_bag_max_workspace_bytes(int64_t nnz, int64_t B, int64_t D);
int ttemb_bag_max(const float* rows, const int64_t* indices /* NULL: no padding */, int64_t pad, const int64_t* offsets,
                  int64_t nnz, int64_t B, int64_t D, float* output, int32_t* argmax, void* workspace, int64_t workspace_bytes,
                  void* stream);
int ttemb_bag_max_backward(const float* d_output, const int32_t* argmax, const int64_t* offsets, int64_t nnz, int64_t B,
                           int64_t D, float* d_rows, void* stream);

/* ---------------------------------------------------------------------------------
 * Padding (torch.nn.functional.embedding_bag's padding_idx: an id equal to `pad` -- compared with the raw id, before any
 * clamping of invalid ids -- adds nothing to its bag, is not counted in a mean and sends no gradient).  Two routes:
 *   - ttemb_drop_padding: a stable flagged partition of indices[0:nnz].  The kept ids -- inside a bag of `offsets`
 *     (int64[B+1]) and != pad -- come first in input order, rowidx_out[i] is the bag of kept id i, and the others fill the
 *     tail from the end backwards (the order of ttemb_preprocess).  offsets_out[b] (int64[B+1]) = the kept ids before
 *     offsets[b]: the compacted bags.  *nnz_kept_dev (int32) = the kept count, left on the device.  Then the lookup runs
 *     on (indices_out, rowidx_out, offsets_out, nnz, nnz_kept_dev) -- pass offsets_out, never the original offsets: a bag
 *     of one pad id has no writer -- and a mean divides by offsets_out's lengths.  Integer work only, no waits between
 *     workgroups (deterministic by construction), grids capped by ttemb_set_exact_grid.  The workspace
 *     (ttemb_drop_padding_workspace_bytes) is used behind the 40 KB header, so the lookups' workspace serves it.
 *   - ttemb_pad_weights (the masked-rows route, with the bags-of-one lookup + ttemb_bag_reduce above):
 *     weights_out[i] = keep[i] * (weights ? weights[i] : 1) * (mean ? 1 / len'(bag(i)) : 1), len' the kept ids of the bag
 *     (0 for a bag without one); 0 for positions outside every bag.  weights may be NULL.  Deterministic likewise.
 * No host synchronisation and no allocation.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_drop_padding_workspace_bytes(int64_t nnz, int64_t B);
int ttemb_drop_padding(const int64_t* indices, const int64_t* offsets, int64_t nnz, int64_t B, int64_t pad,
                       int64_t* indices_out, int64_t* rowidx_out, int64_t* offsets_out, int32_t* nnz_kept_dev, void* workspace,
                       int64_t workspace_bytes, void* stream);
int ttemb_pad_weights(const int64_t* indices, const int64_t* offsets, const float* weights, int64_t nnz, int64_t B,
                      int64_t pad, int32_t mean, float* weights_out, void* stream);

#ifdef __cplusplus
}
#endif

/* Captured pooled lookups -- the staging launch of a pooled call and the pooling calls that take a device id count -- are
 * declared in ttemb_bags.h, which this header includes: one include serves the whole ABI. */
#include "ttemb_bags.h"
#include "ttemb_pads.h"
#include "ttemb_unique.h"
#include "ttemb_unique_n.h"

#endif /* TTEMB_H_ */
