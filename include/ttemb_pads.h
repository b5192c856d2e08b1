/*
 * ttemb_pads.h -- the part of the C ABI of libttemb_hip.so that drops the pad ids of captured PADDED bags on the device
 * (capture_bags(..., pad_route="partition")): a compaction that reads a device id count and carries the weights along, and
 * the way back for the weight gradient.  Included by ttemb.h -- include that; the conventions (error codes, streams, no
 * allocation, no host synchronisation) are stated there.  Additive symbols: TTEMB_ABI_VERSION stays what ttemb.h says.  The
 * declarations live in a header of their own because the sets ttemb.h and ttemb_bags.h declare are pinned by tests.
 */
#ifndef TTEMB_PADS_H_
#define TTEMB_PADS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * ttemb_compact_bags: the stable compaction of ttemb_drop_padding as the FIRST node of a captured forward graph.  With
 * c = min(nnz, max(*nnz_dev, 0)) -- c = nnz for nnz_dev = NULL, the lookups' convention; nnz is the capacity and sizes the
 * launches -- position n is KEPT when n < c, n lies inside [clamp(offsets[0]), clamp(offsets[B])) (both clamped to [0, c])
 * and indices[n] != pad (the raw id, before any clamping of invalid ids): ttemb_drop_padding's rule for nnz = c.
 *     indices_out[0 : kept]   the kept ids, in input order
 *     weights_out[0 : kept]   their weights; weights (float32[nnz]) and weights_out are both given or both NULL
 *     offsets_out[b]          the kept ids before clamp(offsets[b], c), for all B + 1 words: the compacted bags
 *     map_out[n], n < c       (int32, nullable) the compacted position of n, or -1 when n was dropped
 *     *kept_dev               (int32) the kept count: the count word of everything that runs on the compacted buffers
 * Positions >= c of indices / weights are not read; nothing past `kept` of indices_out / weights_out and nothing past c of
 * map_out is written (ttemb_drop_padding fills the tail with the dropped ids; here nobody reads it).  Integer and copy work
 * only, tiles of 256 positions in grid-stride loops (grids capped by ttemb_set_exact_grid), no waits between workgroups,
 * two launches.  The workspace (ttemb_compact_bags_workspace_bytes of nnz) is used behind the 40 KB header, so the lookups'
 * workspace serves it.  TTEMB_E_BADARG, with nothing launched, for a negative size, nnz >= 2^31, a null buffer, weights on
 * one side only and indices_out == indices; TTEMB_E_WORKSPACE for a workspace that is too small.
 * ------------------------------------------------------------------------------- */
int64_t ttemb_compact_bags_workspace_bytes(int64_t nnz);
int ttemb_compact_bags(const int64_t* indices, const int64_t* offsets, const float* weights /* nullable */, int64_t nnz,
                       const int32_t* nnz_dev /* nullable */, int64_t B, int64_t pad, int64_t* indices_out,
                       int64_t* offsets_out, float* weights_out /* NULL exactly when weights is */,
                       int32_t* map_out /* nullable */, int32_t* kept_dev, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------
 * ttemb_expand_kept: the way back.  For n < c (c as above): out[n] = map[n] >= 0 ? src[map[n]] : 0 -- the weight gradient
 * of the compacted positions at the positions of the call, exactly 0 at a dropped one.  A gather: no scatter, no atomics,
 * no memset; positions >= c are neither read nor written.  One launch.  src, map and out hold nnz elements; TTEMB_E_BADARG,
 * with nothing launched, for a negative nnz, nnz >= 2^31, a null buffer and out == src.
 * ------------------------------------------------------------------------------- */
int ttemb_expand_kept(const float* src, const int32_t* map, int64_t nnz, const int32_t* nnz_dev /* nullable */, float* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTEMB_PADS_H_ */
