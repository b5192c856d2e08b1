#!/usr/bin/env python3
"""Pin the library's host-side route decisions: tests/golden/route_table.npz.

Every row is one size query -- forced path x shape x (nnz, B) x piece limits -- and holds what the library answers:
ttemb_workspace_bytes for the four ops, ttemb_plan_bytes, ttemb_kernel_family with and without offsets and
ttemb_window_workspace_bytes for a forward and a backward window of B bags out of 2 B.  A query that fails records -1.
Nothing is launched.

Some numbers follow the device's CU count (the grouping pass's slices, the wide backward's slab shares): the table is
taken with no device visible, where the library assumes 256 CUs (an MI355X's count).  Run it that way:

    HIP_VISIBLE_DEVICES=-1 ROCR_VISIBLE_DEVICES=-1 python tests/golden/make_route_table.py

(TTEMB_LIB selects another build of the library.)
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "route_table.npz")

# 3-core: the q list of test_size_queries_over_every_shape_and_size, over products / papers / large-p2 / degenerate tables
Q3 = ([4, 5, 5], [4, 4, 8], [8, 4, 4], [5, 4, 5], [5, 5, 4], [4, 4, 4], [2, 2, 4], [16, 4, 2])
R3 = (4, 8, 12, 16, 24, 32, 48, 64, 128, 256)
P3 = ([125, 140, 140], [400, 500, 600], [3, 2, 5000], [1, 1, 1], [7, 300, 900])
# 2- and 4-core tables, each with a small and a large first pair
OTHER = (
    ([50, 60], [8, 16], [16]), ([3000, 4000], [8, 16], [16]),
    ([50, 60], [4, 25], [32]), ([3000, 4000], [4, 25], [32]),
    ([40, 50], [10, 10], [64]), ([2000, 3000], [10, 10], [64]),
    ([50, 60, 60, 60], [2, 4, 4, 4], [16, 16, 16]), ([300, 400, 60, 60], [2, 4, 4, 4], [16, 16, 16]),
    ([700, 800, 60, 60], [2, 4, 4, 4], [16, 16, 16]),
    ([10, 12, 30, 40], [2, 2, 5, 5], [16, 16, 16]), ([600, 700, 30, 40], [2, 2, 5, 5], [16, 16, 16]),
    ([10, 12, 30, 40], [5, 5, 2, 2], [16, 16, 16]), ([600, 700, 30, 40], [5, 5, 2, 2], [16, 16, 16]),
    ([7, 9, 11, 5], [2, 2, 5, 4], [5, 6, 3]), ([700, 900, 11, 5], [2, 2, 5, 4], [5, 6, 3]),
)
SIZES = ((0, 0), (1, 1), (100, 100), (5000, 5000), (65536, 65536), (409600, 409600), (819200, 819200),
         (2400000, 2400000), (6000000, 100))
PIECES = ((0, 0), (1000, 2000))   # the hardware's limits; small pieces
COLUMNS = ("ws_forward", "ws_backward", "ws_cache_populate", "ws_preprocess", "plan_bytes", "family_offsets",
           "family_no_offsets", "window_forward", "window_backward")


def shapes():
    for q in Q3:
        for r in R3:
            for p in P3:
                yield p, q, [r, r]
    yield from OTHER


def sweep():
    """-> {"key": int64 [rows, 17] (path, T, p[4], q[4], ranks[3] -- zero-padded --, nnz, B, piece rows, piece ids),
    "value": int64 [rows, len(COLUMNS)]}"""
    pkg = os.path.join(ROOT, "falcon-ttdforgnns_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import ttemb_native as nat
    lib = nat.LIB
    keys, vals = [], []

    def q64(n):
        return -1 if n < 0 else int(n)

    try:
        for piece in PIECES:
            lib.ttemb_set_piece_limits(*piece)
            for path in (nat.PATH_AUTO, nat.PATH_GENERIC, nat.PATH_FAST3, nat.PATH_PER_BAG):
                assert lib.ttemb_set_path(path) == 0
                for p, q, r in shapes():
                    shp = nat.make_shape(p, q, r)
                    ref = ctypes.byref(shp)
                    pad = lambda v, n: list(v) + [0] * (n - len(v))
                    for nnz, B in SIZES:
                        keys.append([path, len(p)] + pad(p, 4) + pad(q, 4) + pad(r, 3)[:3] + [nnz, B, piece[0], piece[1]])
                        vals.append([q64(lib.ttemb_workspace_bytes(ref, nat.OP_FORWARD, nnz, B)),
                                     q64(lib.ttemb_workspace_bytes(ref, nat.OP_BACKWARD, nnz, B)),
                                     q64(lib.ttemb_workspace_bytes(ref, nat.OP_CACHE_POPULATE, nnz, B)),
                                     q64(lib.ttemb_workspace_bytes(ref, nat.OP_PREPROCESS, nnz, B)),
                                     q64(lib.ttemb_plan_bytes(ref, nnz)),
                                     q64(lib.ttemb_kernel_family(ref, nnz, B, 1)),
                                     q64(lib.ttemb_kernel_family(ref, nnz, B, 0)),
                                     q64(lib.ttemb_window_workspace_bytes(ref, nat.OP_FORWARD, nnz, 2 * B, B)),
                                     q64(lib.ttemb_window_workspace_bytes(ref, nat.OP_BACKWARD, nnz, 2 * B, B))])
    finally:
        lib.ttemb_set_path(nat.PATH_AUTO)
        lib.ttemb_set_piece_limits(0, 0)
    return {"key": np.array(keys, dtype=np.int64), "value": np.array(vals, dtype=np.int64)}


if __name__ == "__main__":
    import torch
    assert torch.cuda.device_count() == 0, "take the table with no device visible (see the docstring)"
    t = sweep()
    np.savez_compressed(OUT, columns=np.array(COLUMNS), **t)
    print(f"{OUT}: {len(t['key'])} rows")
