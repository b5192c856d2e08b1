/*
 * ttemb_unique.h -- the part of the C ABI of libttemb_hip.so that serves the `dedup` route of the pooled lookups: the pass
 * that finds the distinct ids of a call on the device, and the pooling calls that read the looked-up rows through the map
 * that pass writes.  Included by ttemb.h -- include that; the conventions (error codes, streams, no
 * allocation, no host synchronisation) are stated there.  Additive symbols: TTEMB_ABI_VERSION stays what ttemb.h says.  The
 * declarations live in a header of their own because the sets ttemb.h, ttemb_bags.h and ttemb_pads.h declare are pinned by
 * tests.
 */
#ifndef TTEMB_UNIQUE_H_
#define TTEMB_UNIQUE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * ttemb_unique_ids: the distinct ids of indices[0 : nnz], on the device.  With U their number:
 *     unique_out[0 : U]     the distinct ids in ascending order (torch.unique(sorted=True))
 *     inverse_out[n]        (int32) the place of indices[n] in unique_out, for every n < nnz (return_inverse)
 *     perm_out[0 : nnz]     (int32) the positions 0 .. nnz-1 sorted by id, equal ids in ascending position (stable)
 *     seg_out[j], j <= U    where the positions of unique_out[j] begin in perm_out; seg_out[U] = nnz
 *     *count_dev            (int32) U: the count word of everything that runs on the distinct ids
 * unique_out[U : nnz] and seg_out[U + 1 : nnz + 1] are NOT written (they keep what they held) and nobody reads them.
 *
 * `rows` is the number of rows of the table: the ids are sorted by a stable radix sort on the key bits
 * [0, bit_length(rows - 1)), then the heads of the runs of equal ids are flagged by comparing the full 64-bit ids, counted
 * per tile of 256 sorted positions and scattered.  An id outside [0, rows) is as undefined for the lookup as it is without
 * this pass (equal ids may then end up in more than one run), but for ANY int64 content the pass reads and writes nothing
 * outside its buffers: U <= nnz, inverse_out[n] < U, seg_out is ascending.
 *
 * Integer work only; the sort is rocprim's, out of the workspace; two hand-written launches behind it (tiles of 256 in
 * grid-stride loops, grids capped by ttemb_set_exact_grid, no waits between workgroups).  The results do not depend on the
 * grid.  The workspace (ttemb_unique_ids_workspace_bytes of the same nnz and rows, negative on an error) is used behind the
 * 40 KB header, so the lookups' workspace serves it; it owns nothing past the call -- the five outputs are the caller's.
 *
 * nnz is known on the host (eager calls).  TTEMB_E_BADARG, with nothing launched, for a negative nnz, nnz >= 2^31,
 * rows <= 0 and a null buffer (unique_out / inverse_out / perm_out / indices may be NULL when nnz == 0);
 * TTEMB_E_WORKSPACE for a workspace that is too small.  nnz == 0 is valid: U = 0, seg_out[0] = 0.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_unique_ids_workspace_bytes(int64_t nnz, int64_t rows);
int ttemb_unique_ids(const int64_t* indices, int64_t nnz, int64_t rows,
                     int64_t* unique_out /* [nnz] */, int32_t* inverse_out /* [nnz] */,
                     int32_t* perm_out /* [nnz] */, int64_t* seg_out /* [nnz + 1] */,
                     int32_t* count_dev /* [1] */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * ttemb_bag_reduce_mapped: ttemb_bag_reduce reading its rows through a map.
 *     output[b] = sum_{n in bag b} w[n] rows[map[n]],  n in position order,  w = 1 for weights == NULL
 * rows is [cap][D] (cap >= 1 when nnz > 0), map int32 [nnz]; a map word outside [0, cap) is clamped into it, so no content of
 * map can send a load astray.  The same 512-position chunks and chunk-order partial sums as ttemb_bag_reduce (and its
 * workspace: ttemb_bag_workspace_bytes(nnz, B, D)): for equal rows[map[n]] bits it gives the bits ttemb_bag_reduce gives on
 * the expanded [nnz][D] rows (with weights == NULL: those of weights of 1.0f).  output is written for all B bags.  Checks and
 * error codes as ttemb_bag_reduce, plus TTEMB_E_BADARG for cap < 1 with nnz > 0, nnz >= 2^31 and a null map.
 * ------------------------------------------------------------------------------- */
int ttemb_bag_reduce_mapped(const float* rows, int64_t cap, const int32_t* map, const float* weights /* nullable: 1 */,
                            const int64_t* offsets, int64_t nnz, int64_t B, int64_t D, float* output, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * ttemb_bag_reduce_mapped_backward: the gradient of the above.  perm / seg / count_dev are ttemb_unique_ids' outputs for the
 * ids map was made from; U = min(nnz, max(*count_dev, 0)).
 *     d_rows[j], j < U      = sum_{k in [seg[j], seg[j+1])} w[perm[k]] d_output[bag(perm[k])],  summed in k order; a
 *                             position outside every bag contributes zero.  A segment of more than 512 positions is cut
 *                             into the fixed chunks [512 m, 512 (m+1)) of the SORTED position list and its partials are
 *                             added in chunk order: the long-bag scheme of ttemb_bag_reduce with seg in the role of offsets.
 *     d_weights[n], n < nnz = <d_output[bag(n)], rows[map[n]]>  (nullable; needs rows, [cap][D]); 0 outside every bag.
 * The bag of every position is found once, one thread per position, into the workspace (int32 [nnz], -1 outside every bag);
 * the sums read it.  The workspace is ttemb_bag_workspace_bytes(nnz, B, D) + 4 nnz bytes rounded up to a multiple of 256 (the
 * chunk partials, then that array).  The launches are sized by nnz; the kernels stop at U: no row >= U of d_rows (which holds
 * at least min(nnz, cap) rows) is written or read.  perm and seg words are clamped into [0, nnz) /
 * [0, nnz] before use.  No float atomics, no waits between workgroups; the summation orders depend on seg and D alone.
 * TTEMB_E_BADARG, with nothing launched, for what ttemb_bag_reduce_backward refuses, nnz >= 2^31, B >= 2^31, cap < 1 with
 * nnz > 0 and a null map / perm / seg / count_dev; TTEMB_E_WORKSPACE for a workspace that is too small.
 * ------------------------------------------------------------------------------- */
int ttemb_bag_reduce_mapped_backward(const float* d_output, const float* weights /* nullable: 1 */,
                                     const float* rows /* NULL: no d_weights */, int64_t cap, const int32_t* map,
                                     const int32_t* perm, const int64_t* seg, const int32_t* count_dev,
                                     const int64_t* offsets, int64_t nnz, int64_t B, int64_t D, float* d_rows,
                                     float* d_weights /* nullable */, void* workspace, int64_t workspace_bytes,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTEMB_UNIQUE_H_ */
