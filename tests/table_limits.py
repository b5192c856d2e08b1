"""Tables on the size limits the kernel dispatch states, and call inputs that put ids on those limits (shared by
test_table_limits_host.py and test_gpu_table_limits.py; numpy only).

The limits (falcon-ttdforgnns_amd/csrc/): the grouped kernels and the per-bag kernels hold ids in 32 bits (``classify`` /
``wide`` in ttemb_fast3.hip, ``small3_only`` in ttemb_small3.inc, ``rt3_supported`` in ttemb_rt3.inc: rows < 2^31 - 1);
``fits_shape`` in ttemb_fast3.hip keeps the grouped kernels to p2 <= 4096, p1 < 65536, G = p0 p1 <= 512 * 4096 groups and
G q0 q1 R2 4 < 2^31 bytes of prefix products.  The exact kernels (``exact_shape`` in ttemb_exact.hip) and the scalar kernels
decode 64-bit ids.  Every "edge" table below sits on one limit, the "over" table beside it one step past it."""
import numpy as np

import fp32_bound as fb

Q455, Q448, Q554, Q644 = [4, 5, 5], [4, 4, 8], [5, 5, 4], [6, 4, 4]

# name -> (p, q, inner ranks).  Where a limit concerns only G = p0 p1 the large factor sits in p0, so that core 1 (p1 rows of
# R1 q1 R2 floats) and its float64 oracle copies stay small; "*_as_stated" is the orientation with the large factor in p1.
TABLES = {
    "rows_edge": ([93, 10923, 2114], Q455, [16, 16]),            # 2^31 - 2 rows: the last table with 32-bit ids
    "rows_edge_as_stated": ([31, 32769, 2114], Q455, [16, 16]),  # 2^31 - 2 rows
    "rows_over": ([1024, 1024, 2048], Q455, [16, 16]),           # 2^31 rows
    "rows_far_over": ([2048, 1024, 4096], Q455, [16, 16]),       # 2^33 rows
    "rows_edge_rt": ([93, 10923, 2114], Q644, [16, 16]),         # 2^31 - 2 rows on the run-time-shape per-bag kernels
    "p2_edge": ([20, 30, 4096], Q455, [16, 16]),                 # p2 = 4096: a 12-bit i2 in the sort key
    "p2_over": ([20, 30, 4097], Q455, [16, 16]),
    "p1_edge": ([2, 65535, 16], Q448, [8, 8]),                   # p1 = 65535: the largest grid.y extent
    "p1_over": ([2, 65536, 16], Q448, [8, 8]),
    "groups_edge": ([512, 4096, 4], Q448, [8, 8]),               # G = 2^21: 512 ranges of 2^12 groups
    "groups_ragged": ([509, 4099, 4], Q448, [8, 8]),             # G = 2 086 391: 510 ranges, the last one holds 1 527 groups
    "groups_over": ([513, 4096, 4], Q448, [8, 8]),               # G = 2^21 + 4096
    "bytes_edge": ([54120, 31, 5], Q455, [16, 16]),              # G * 1280 B = 2^31 - 2048
    "bytes_edge_as_stated": ([31, 54120, 5], Q455, [16, 16]),
    "bytes_over": ([54121, 31, 5], Q455, [16, 16]),              # G * 1280 B = 2^31 + 37 632
    "bytes_over_as_stated": ([31, 54121, 5], Q455, [16, 16]),
    "wide_edge": ([41943, 8, 8], Q554, [64, 64]),                # G * 6400 B = 2^31 - 2048
    "wide_edge_as_stated": ([8, 41943, 8], Q554, [64, 64]),
    "wide_over": ([41944, 8, 8], Q554, [64, 64]),                # G * 6400 B = 2^31 + 49 152
    "wide_over_as_stated": ([8, 41944, 8], Q554, [64, 64]),
}


def rows_of(p):
    n = 1
    for x in p:
        n *= int(x)
    return n


def limit_ids(p):
    """The ids of a 3-core table that sit on its limits, without repeats: 0, rows - 1, rows - 2; the first and the last row
    of the last group (i0 = p0 - 1, i1 = p1 - 1); i2 = p2 - 1 in the first and in the last group; i2 = 0 with i1 = p1 - 1
    (i0 = 0 and i0 = p0 - 1); one id in each of the last three groups, in the order of the ids (i0 p1 + i1) and in the order
    the grouping pass numbers them (i1 p0 + i0); and, where the table has them, the ids around 2^31 and 2^32."""
    p0, p1, p2 = (int(x) for x in p)
    rows, G = p0 * p1 * p2, p0 * p1
    at = lambda i0, i1, i2: (i0 * p1 + i1) * p2 + i2
    ids = [0, rows - 1, rows - 2, at(p0 - 1, p1 - 1, 0), at(p0 - 1, p1 - 1, p2 - 1), at(0, 0, p2 - 1), at(0, p1 - 1, 0)]
    for k in range(1, min(3, G) + 1):
        ids.append(at((G - k) // p1, (G - k) % p1, min(1, p2 - 1)))
        ids.append(at((G - k) % p0, (G - k) // p0, min(2, p2 - 1)))
    ids += [x for x in (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1) if x < rows]
    assert all(0 <= x < rows for x in ids)
    return list(dict.fromkeys(ids))


def place_limit_ids(ids, offs, special):
    """Overwrite positions of ``ids`` (in place) so that every id of ``special`` stands once alone in a one-id bag and once
    inside a bag of several ids (at its first, a middle or its last position in turn); ``special[1]`` (rows - 1 in
    ``limit_ids``' order) stands twice more in the longest bag, next to itself.  The bags stay as they are."""
    lens = np.diff(offs)
    single = np.flatnonzero(lens == 1)
    multi = np.flatnonzero((lens >= 2) & (lens <= 7))
    assert single.size >= len(special) and multi.size >= len(special), "too few bags for the ids on the limits"
    s_step, m_step = single.size // len(special), multi.size // len(special)
    for k, x in enumerate(special):
        ids[offs[single[k * s_step]]] = x
        b = multi[k * m_step]
        ids[offs[b] + (0, lens[b] // 2, lens[b] - 1)[k % 3]] = x
    longest = int(np.argmax(lens))
    if lens[longest] >= 4:
        ids[offs[longest] + 1:offs[longest] + 3] = special[1]
    return ids


# The calls test_gpu_table_limits.py makes, one per case: key -> (table, ids asked of fb.skewed_bags, seed).  Kept here so that
# test_table_limits_host.py checks, without a device, the very ids the GPU cases use.
EDGE_TABLES = ("rows_edge", "p2_edge", "p1_edge", "groups_edge", "groups_ragged", "bytes_edge", "wide_edge")
OVER_TABLES = ("rows_over", "rows_far_over", "p2_over", "p1_over", "groups_over", "bytes_over", "wide_over")
CALLS = {t: (t, 4000 if t == "wide_edge" else 6000, len(t)) for t in EDGE_TABLES}
CALLS.update({f"{t}_{path}": (t, 4000, len(t) + len(path)) for t in OVER_TABLES for path in ("fast3", "auto")})
CALLS.update({f"{t}_{path}": (t, 4000, len(t) + len(path)) for t in ("rows_edge", "rows_edge_rt") for path in ("auto", "per_bag")})
CALLS.update({f"{t}_exact": (t, 6000, len(t)) for t in ("rows_over", "rows_far_over")})


def call_ids(p, n_ids, seed, long_bag=600):
    """(ids, offsets, the generator after them): fb.skewed_bags' ids with the ids of ``limit_ids`` placed among them."""
    rng = np.random.default_rng(seed)
    ids, offs = fb.skewed_bags(rng, p, n_ids, long_bag)
    place_limit_ids(ids, offs, limit_ids(p))
    return ids, offs, rng


def call_inputs(p, q, R, n_ids, seed, long_bag=600):
    """(cores, ids, offsets, dY, Adagrad state): ``call_ids``, then fb.scaled_cores / fb.scaled_dy as in
    test_gpu_accuracy.py from the same generator."""
    ids, offs, rng = call_ids(p, n_ids, seed, long_bag)
    cores = fb.scaled_cores(rng, p, q, R)
    dy = fb.scaled_dy(rng, offs.shape[0] - 1, int(np.prod(q)))
    st0 = [(rng.random(c.shape) * 1e-6).astype(np.float32) for c in cores]
    return cores, ids, offs, dy, st0
