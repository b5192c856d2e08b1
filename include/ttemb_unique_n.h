/*
 * ttemb_unique_n.h -- the part of the C ABI of libttemb_hip.so that puts the `dedup` route of the pooled lookups into a
 * captured graph (capture_bags(..., dedup=True)): the calls of ttemb_unique.h behind a DEVICE id count,
 * as ttemb_bag_reduce_n stands to ttemb_bag_reduce.  Included by ttemb.h -- include that; the conventions (error codes,
 * streams, no allocation, no host synchronisation) are stated there.  Additive symbols: TTEMB_ABI_VERSION stays what ttemb.h
 * says.  The declarations live in a header of their own because the sets ttemb.h, ttemb_bags.h, ttemb_pads.h and
 * ttemb_unique.h declare are pinned by tests.
 */
#ifndef TTEMB_UNIQUE_N_H_
#define TTEMB_UNIQUE_N_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * ttemb_unique_ids_n: ttemb_unique_ids of the first n ids of a buffer of nnz_cap, n = min(nnz_cap, max(*nnz_dev, 0)) read
 * on the device (nnz_dev = NULL: n = nnz_cap, the lookups' convention).  With U the number of distinct ids among
 * indices[0 : n], the outputs are bit for bit those of ttemb_unique_ids(indices, n, rows, ...):
 *     unique_out[0 : U], inverse_out[0 : n], perm_out[0 : n], seg_out[0 : U + 1] (seg_out[U] = n), *count_dev = U
 * unique_out[U :], inverse_out[n :] and seg_out[U + 1 :] are NOT written; perm_out[n : nnz_cap] is overwritten (with the
 * dead positions) and nobody reads it.  indices[n : nnz_cap] -- what earlier calls left there -- influences no output.
 *
 * The launches and the temporary storage of the sort are sized by nnz_cap alone, and nothing the host does depends on n:
 * the call can be captured into a graph once and replayed for every n.  A key launch writes (id & mask) for a position
 * below n and 1 << key_bits(rows) for one at or past it; the stable pair sort of ttemb_unique_ids then runs over
 * key_bits + 1 bits, so every dead position sorts behind every live one and the live part of the sorted positions is what
 * the sort of n ids gives.  The count and scatter launches stop at n and compare the full 64-bit ids, read through the sorted
 * positions.  As in ttemb_unique_ids: for ANY int64 content nothing is read or written outside the buffers (U <= n,
 * inverse_out[.] < U, seg_out ascending and <= n); integer work only, tiles of 256 in grid-stride loops, grids capped by
 * ttemb_set_exact_grid, no waits between workgroups, results independent of the grid.
 *
 * The workspace (ttemb_unique_ids_n_workspace_bytes of the same nnz_cap and rows, negative on an error; more than
 * ttemb_unique_ids needs: the keys have a buffer of their own) is used behind the 40 KB header.  Up to 2^20 ids the sort
 * consists of kernels only; past that it also clears its counters with memset nodes when it is captured.
 *
 * TTEMB_E_BADARG, with nothing launched, for a negative nnz_cap, nnz_cap >= 2^31, rows <= 0 and a null buffer (unique_out /
 * inverse_out / perm_out / indices may be NULL when nnz_cap == 0); TTEMB_E_WORKSPACE for a workspace that is too small.
 * n == 0 is valid: U = 0, seg_out[0] = 0.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_unique_ids_n_workspace_bytes(int64_t nnz_cap, int64_t rows);
int ttemb_unique_ids_n(const int64_t* indices, int64_t nnz_cap, const int32_t* nnz_dev /* nullable */, int64_t rows,
                       int64_t* unique_out /* [nnz_cap] */, int32_t* inverse_out /* [nnz_cap] */,
                       int32_t* perm_out /* [nnz_cap] */, int64_t* seg_out /* [nnz_cap + 1] */,
                       int32_t* count_dev /* [1] */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * ttemb_bag_reduce_mapped_n / ttemb_bag_reduce_mapped_backward_n: the two pooling calls of ttemb_unique.h with
 * `const int32_t* nnz_dev` behind nnz.  With n = min(nnz, max(*nnz_dev, 0)) (NULL: n = nnz) every kernel uses n where the
 * parent uses nnz: bags and segments are clamped to n, no map / weights / perm word at a position >= n is read, no
 * d_weights[p >= n] and no d_rows row >= U = min(n, cap, max(*count_dev, 0)) is written, while the launches, the checks and
 * the workspace stay sized by nnz, the capacity.  On the live part the bits are those of the parent called with nnz = n;
 * ttemb_bag_reduce_mapped and ttemb_bag_reduce_mapped_backward ARE these calls with nnz_dev = NULL.  Error codes as theirs.
 * ------------------------------------------------------------------------------- */
int ttemb_bag_reduce_mapped_n(const float* rows, int64_t cap, const int32_t* map, const float* weights /* nullable: 1 */,
                              const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B,
                              int64_t D, float* output, void* workspace, int64_t workspace_bytes, void* stream);
int ttemb_bag_reduce_mapped_backward_n(const float* d_output, const float* weights /* nullable: 1 */,
                                       const float* rows /* NULL: no d_weights */, int64_t cap, const int32_t* map,
                                       const int32_t* perm, const int64_t* seg, const int32_t* count_dev,
                                       const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev, int64_t B,
                                       int64_t D, float* d_rows, float* d_weights /* nullable */, void* workspace,
                                       int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTEMB_UNIQUE_N_H_ */
