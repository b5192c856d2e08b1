/*
 * ttemb_bags.h -- the part of the C ABI of libttemb_hip.so that serves captured POOLED lookups (weighted, mean, max,
 * padded and fixed-fanout bags inside HIP graphs): one staging launch and the pooling calls of ttemb.h with a device id
 * count.  Included by ttemb.h -- include that; the conventions (error codes, streams, no allocation, no host
 * synchronisation) are stated there.  Additive symbols: TTEMB_ABI_VERSION stays what ttemb.h says.  The declarations live
 * in a header of their own because the set ttemb.h declares is pinned by the tests of the device-resident learning rate.
 */
#ifndef TTEMB_BAGS_H_
#define TTEMB_BAGS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * Stage one POOLED call into the static buffers of captured bags ("Count-aware pooling" below): ttemb_stage_call plus
 * per-sample weights and bags of a fixed fanout.  Everything ttemb_stage_call writes is written identically; ONE launch,
 * no host synchronisation, no workspace.  In addition:
 *     weights_in (nullable)  float32 [n_live]: weights_out[0 : n_live] = weights_in; weights_out[n_live :] is NOT touched.
 *                            weights_in and weights_out are both given or both NULL.
 *     fanout == 0            offsets as ttemb_stage_call (offsets_in, or NULL: bags of one id).
 *     fanout  > 0            the 2-D call indices[B_live][fanout]: offsets_in must be NULL and n_live == B_live * fanout;
 *                            offsets_out[b] = b * fanout for b <= B_live, n_live in every word past them -- generated on
 *                            the device: no host-side arange, no CSR.
 * TTEMB_E_BADARG, with nothing launched, for every case ttemb_stage_call refuses, weights on one side only, fanout < 0, and
 * fanout > 0 with offsets_in or with n_live != B_live * fanout.
 * ------------------------------------------------------------------------------- */
int ttemb_stage_bags(const void* indices_in, int32_t indices_are_i32, int64_t n_live,
                     const void* offsets_in /* nullable */, int32_t offsets_are_i32, int64_t B_live, int64_t fanout,
                     const float* weights_in /* nullable */,
                     int64_t* indices_out, int64_t nnz_cap,
                     int64_t* offsets_out, int64_t B_cap,
                     float* weights_out /* NULL exactly when weights_in is */,
                     int32_t* nnz_dev_out, void* stream);

/* ---------------------------------------------------------------------------------
 * Count-aware pooling: the pooling calls above with a device id count, for HIP graphs captured at a capacity
 * (ttemb_stage_bags in front of the replay).  Each is the signature of its namesake plus `nnz_dev` (int32 on the device,
 * nullable) behind `nnz`, the convention of the lookups: with c = min(nnz, max(*nnz_dev, 0)) -- c = nnz for NULL -- every
 * kernel uses c where its namesake uses nnz.  Bags are clamped to c; the loops over positions and over the 512-id chunks
 * stop at c; positions >= c of rows / weights / indices are not read and those of d_rows, d_weights and weights_out are
 * neither read nor written.  output / argmax are written for all B bags (a bag past the live ids is empty: zeros, -1).
 * The launches and the workspaces (ttemb_bag_workspace_bytes / ttemb_bag_max_workspace_bytes of nnz) are sized by nnz, the
 * capacity.  Chunks are cut from position 0, so the live part is bit for bit what the namesake gives for nnz = c with the
 * same offsets; the calls without the suffix ARE these calls with nnz_dev = NULL.  Checks and error codes as the namesakes
 * (on nnz, before any launch).  ttemb_bag_mean needs no count: the bags past the live ones are empty and get zeros.
 * ------------------------------------------------------------------------------- */
int ttemb_bag_reduce_n(const float* rows, const float* weights, const int64_t* offsets, int64_t nnz,
                       const int32_t* nnz_dev /* nullable */, int64_t B, int64_t D, float* output, void* workspace,
                       int64_t workspace_bytes, void* stream);
int ttemb_bag_reduce_backward_n(const float* d_output, const float* weights, const float* rows /* NULL: no d_weights */,
                                const int64_t* offsets, int64_t nnz, const int32_t* nnz_dev /* nullable */, int64_t B,
                                int64_t D, float* d_rows, float* d_weights /* NULL: no weight gradient */, void* workspace,
                                int64_t workspace_bytes, void* stream);
int ttemb_bag_max_n(const float* rows, const int64_t* indices /* NULL: no padding */, int64_t pad, const int64_t* offsets,
                    int64_t nnz, const int32_t* nnz_dev /* nullable */, int64_t B, int64_t D, float* output, int32_t* argmax,
                    void* workspace, int64_t workspace_bytes, void* stream);
int ttemb_bag_max_backward_n(const float* d_output, const int32_t* argmax, const int64_t* offsets, int64_t nnz,
                             const int32_t* nnz_dev /* nullable */, int64_t B, int64_t D, float* d_rows, void* stream);
int ttemb_pad_weights_n(const int64_t* indices, const int64_t* offsets, const float* weights, int64_t nnz,
                        const int32_t* nnz_dev /* nullable */, int64_t B, int64_t pad, int32_t mean, float* weights_out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTEMB_BAGS_H_ */
