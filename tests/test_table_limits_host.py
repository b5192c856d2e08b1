"""CPU: the route the library decides for the tables of tests/table_limits.py, on each size limit of the kernel families and
one step past it.  The expectations are literals: a change of a predicate (``classify`` / ``wide`` / ``fits_shape`` in
ttemb_fast3.hip, ``small3_only``, ``rt3_supported``, ``exact_shape``) has to edit this file on purpose.  The queries run in a
child process with no device visible, as in test_grouping_buckets_host.py; test_gpu_table_limits.py runs the same tables."""
import json
import os
import subprocess
import sys

import table_limits as tl
from conftest import ROOT

NNZ, BAGS = 20000, 10000

CODE = r"""
import sys, json
import torch
assert torch.cuda.device_count() == 0, 'the device is not hidden'
import ttemb_native as nat
tables, nnz, B = json.loads(sys.argv[1])
out = {}
for name, (p, q, r) in tables.items():
    s = nat.make_shape(p, q, r)
    row = {}
    for key, path in (("fast3", nat.PATH_FAST3), ("auto", nat.PATH_AUTO), ("per_bag", nat.PATH_PER_BAG)):
        nat.set_path(path)
        row[key] = {"family": nat.kernel_family(s, nnz, B, True), "plan": nat.plan_bytes(s, nnz),
                    "ws": [nat.workspace_bytes(s, op, nnz, B) for op in (nat.OP_FORWARD, nat.OP_BACKWARD)]}
    nat.set_path(nat.PATH_AUTO)
    try:
        row["ranges"] = nat.grouping_layout(s, nnz)["ranges"]
    except RuntimeError as e:   # (only the refusal of a shape without grouped kernels is an answer)
        if "no grouped kernels for this shape" not in str(e):
            raise
        row["ranges"] = None
    row["exact"] = nat.exact_unsupported_reason(s)
    out[name] = row
print(json.dumps(out))
"""

GROUPED, WIDE, PREFIX, PRODUCTS = 3, 4, 64, 128   # FAMILY_GROUPED, _GROUPED_WIDE, _PREFIX_IN_CHAIN, _GROUP_PRODUCTS_IN_CHAIN

# table -> (family under PATH_FAST3, PATH_AUTO, PATH_PER_BAG for a call of 20 000 ids in 10 000 bags; edge side (a plan is kept
# under PATH_FAST3); ranges of the grouping pass, None where the query refuses the shape; exact mode covers the table)
EXPECT = {
    # rows < 2^31 - 1 (classify / wide / small3_only / rt3_supported: ids held in 32 bits)
    "rows_edge": (GROUPED | PREFIX | PRODUCTS, 1, 1, True, 497, True),             # 2^31 - 2 rows
    "rows_edge_as_stated": (GROUPED | PREFIX | PRODUCTS, 1, 1, True, 497, True),   # 2^31 - 2 rows
    "rows_over": (0, 0, 0, False, None, True),                                     # 2^31 rows: scalar kernels only
    "rows_far_over": (0, 0, 0, False, None, True),                                 # 2^33 rows
    "rows_edge_rt": (0, 2, 2, False, None, True),                                  # 2^31 - 2 rows, q = 6,4,4: rt3_supported
    # p2 <= 4096 (fits_shape: 12 bits of i2 in the sort key, two LDS counters per i2)
    "p2_edge": (GROUPED, GROUPED, 1, True, 300, True),                             # p2 = 4096
    "p2_over": (0, 1, 1, False, 300, True),                                        # p2 = 4097
    # p1 < 65536 (fits_shape: a grid.y extent)
    "p1_edge": (GROUPED | PREFIX, 1, 1, True, 512, True),                          # p1 = 65535
    "p1_over": (0, 1, 1, False, 512, True),                                        # p1 = 65536
    # p0 p1 <= 512 * 4096 (fits_shape: 512 ranges of at most 2^12 groups)
    "groups_edge": (GROUPED | PREFIX, 1, 1, True, 512, True),                      # G = 2^21
    "groups_ragged": (GROUPED | PREFIX, 1, 1, True, 510, True),                    # G = 2 086 391
    "groups_over": (0, 1, 1, False, 257, True),                                    # G = 2^21 + 4096 (would need shift 13)
    # p0 p1 q0 q1 R2 4 < 2^31 (fits_shape: 32-bit byte offsets into the prefix products)
    "bytes_edge": (GROUPED | PREFIX, 1, 1, True, 410, True),                       # 2^31 - 2048 bytes
    "bytes_edge_as_stated": (GROUPED | PREFIX, 1, 1, True, 410, True),
    "bytes_over": (0, 1, 1, False, 410, True),                                     # 2^31 + 37 632 bytes
    "bytes_over_as_stated": (0, 1, 1, False, 410, True),
    "wide_edge": (WIDE, 1, 1, True, 328, False),                                   # rank 64: 2^31 - 2048 bytes
    "wide_edge_as_stated": (WIDE, 1, 1, True, 328, False),
    "wide_over": (0, 1, 1, False, 328, False),                                     # 2^31 + 49 152 bytes
    "wide_over_as_stated": (0, 1, 1, False, 328, False),
}


def _answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "falcon-ttdforgnns_amd"), ROOT, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", CODE, json.dumps([tl.TABLES, NNZ, BAGS])], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_tables_sit_on_the_limits_they_are_named_for():
    rows = {k: tl.rows_of(v[0]) for k, v in tl.TABLES.items()}
    groups = {k: v[0][0] * v[0][1] for k, v in tl.TABLES.items()}
    prefix_bytes = {k: groups[k] * q[0] * q[1] * r[1] * 4 for k, (p, q, r) in tl.TABLES.items()}
    assert rows["rows_edge"] == rows["rows_edge_as_stated"] == rows["rows_edge_rt"] == 2 ** 31 - 2 == 0x7fffffff - 1
    assert rows["rows_over"] == 2 ** 31 and rows["rows_far_over"] == 2 ** 33
    assert tl.TABLES["p2_edge"][0][2] == 4096 and tl.TABLES["p2_over"][0][2] == 4097
    assert tl.TABLES["p1_edge"][0][1] == 65535 and tl.TABLES["p1_over"][0][1] == 65536
    assert groups["groups_edge"] == 512 * 4096 and groups["groups_over"] == 512 * 4096 + 4096
    assert groups["groups_ragged"] == 2086391 and -(-groups["groups_ragged"] // 4096) == 510
    for k in ("bytes", "wide"):
        assert prefix_bytes[k + "_edge"] == prefix_bytes[k + "_edge_as_stated"] == 2 ** 31 - 2048
        assert 2 ** 31 < prefix_bytes[k + "_over"] == prefix_bytes[k + "_over_as_stated"] < 2 ** 31 + 65536
    for k, (p, q, r) in tl.TABLES.items():   # apart from the limit a table is named for, it is inside every other one
        if not k.startswith("rows_") or k.startswith("rows_edge"):
            assert rows[k] < 2 ** 31 - 1, k
        if not k.startswith("p2_"):
            assert p[2] <= 4096, k
        if not k.startswith("p1_"):
            assert p[1] < 65536, k
        if not k.startswith("groups_"):
            assert groups[k] <= 512 * 4096, k
        if not k.startswith(("bytes_", "wide_")) and k != "rows_far_over":   # (2^33 rows: 2^21 groups of 1280 bytes, too)
            assert prefix_bytes[k] < 2 ** 31, k


def test_routes_on_and_past_the_table_size_limits():
    assert sorted(EXPECT) == sorted(tl.TABLES)
    got = _answers()
    for name, (f_fast3, f_auto, f_per_bag, edge, ranges, exact) in EXPECT.items():
        a = got[name]
        fams = (a["fast3"]["family"], a["auto"]["family"], a["per_bag"]["family"])
        assert fams == (f_fast3, f_auto, f_per_bag), (name, fams)
        if edge:
            assert a["fast3"]["plan"] > 0, (name, a["fast3"])
            assert f_fast3 & 7 in (GROUPED, WIDE), name
        else:
            assert all(a[k]["plan"] == 0 for k in ("fast3", "auto", "per_bag")), (name, a)
            assert all(f & 7 not in (GROUPED, WIDE) for f in fams), (name, fams)
        assert a["per_bag"]["plan"] == 0, name   # the per-bag kernels keep no plan
        for k in ("fast3", "auto", "per_bag"):
            fwd, bwd = a[k]["ws"]
            assert 0 <= fwd <= bwd, (name, k, a[k]["ws"])
        assert a["ranges"] == ranges, (name, a["ranges"])
        assert ranges is None or ranges <= 512, name
        if exact:
            assert a["exact"] is None, (name, a["exact"])
        else:
            assert a["exact"] and "ranks (64, 64)" in a["exact"], (name, a["exact"])


def test_call_inputs_put_ids_on_the_limits_and_stay_inside_the_bound():
    """What test_gpu_table_limits.py relies on, checked without a device on the ids of every call it makes (``tl.CALLS``):
    every id of ``limit_ids`` stands once alone in a bag and once inside a bag of several ids, every core has touched rows,
    and the deepest accumulation of any route stays inside fb.gamma's domain (depth * u < 0.5)."""
    import numpy as np

    import fp32_bound as fb
    from oracle import tt_oracle as orc
    assert {t for t, _, _ in tl.CALLS.values()} == {k for k in tl.TABLES if not k.endswith("_as_stated")}
    for key, (table, n_ids, seed) in tl.CALLS.items():
        p, q, r = tl.TABLES[table]
        R = [1] + r + [1]
        rows = tl.rows_of(p)
        special = tl.limit_ids(p)
        assert {0, rows - 1, rows - 2, p[2] - 1, rows - p[2], (p[1] - 1) * p[2]} <= set(special), key
        if rows > 2 ** 32 + 1:
            assert {2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1} <= set(special), key
        ids, offs, _ = tl.call_ids(p, n_ids, seed)
        assert 4000 <= n_ids <= 8000 and ids.min() == 0 and ids.max() == rows - 1, key
        lens = np.diff(offs)
        bag = np.repeat(np.arange(lens.size), lens)
        for x in special:
            at = lens[bag[ids == x]]
            assert (at == 1).any() and (at > 1).any(), (key, x)
        counts = [np.bincount(d, minlength=p[t]) for t, d in enumerate(orc.split_index(ids, p))]
        for route in (("wide",) if r[0] >= 64 else ("grouped",)) + ("per_bag", "scalar", "exact"):
            fb.gamma(fb.bag_depth(route, R, lens))
            for t in range(3):
                assert counts[t].any(), (key, t)
                fb.gamma(fb.grad_depth(route, q, R, t, counts[t]))
