"""CPU: the grouped path's workspace size query covers the grouping pass's range buckets with slack, plus the worst-case
overflow area (every id in overflow, one block header per (round of a slice, range)), on top of the plan and the header."""
import subprocess
import sys

import numpy as np

from conftest import ROOT

CODE = r"""
import sys, json
import numpy as np
import ttemb_native as nat
P, Q, R = [125, 140, 140], [4, 5, 5], [1, 16, 16, 1]
shape = nat.make_shape(P, Q, R)
out = {}
for n in (8192, 12345, 409600, 819200, 2400000):   # (all grouped: >= 4 375 ids on this table)
    out[n] = [nat.workspace_bytes(shape, nat.OP_FORWARD, n, n), nat.workspace_bytes(shape, nat.OP_BACKWARD, n, n),
              nat.plan_bytes(shape, n), nat.grouping_layout(shape, n)]
print(json.dumps(out))
"""


def _sizes():
    # a child process with no device visible: the library sizes for 256 CUs, as on an MI355X
    import os
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "falcon-ttdforgnns_amd"), ROOT, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", CODE], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    return {int(k): v for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}


def test_workspace_covers_buckets_and_worst_case_overflow():
    """The layout the library uses (ttemb_grouping_layout): buckets of at least 1.5x the uniform fill, an overflow area that
    holds every id plus a block header per (round of a slice, range), and a workspace size query that covers both."""
    a256 = lambda x: (x + 255) // 256 * 256
    G, ranges, header = 125 * 140, 274, 40960
    for n, (fwd, bwd, plan, lay) in _sizes().items():
        slices = min(-(-n // 2048), 256)
        banks = min(slices, 8)
        per_slice = -(-n // slices)
        headers = slices * -(-per_slice // 4096) * ranges
        assert (lay["slices"], lay["ranges"], lay["banks"]) == (slices, ranges, banks), (n, lay)
        assert lay["ovf_slots"] >= n + min(n, headers), (n, lay)               # every id in overflow + a header per (round, range)
        mean = -(-n // (ranges * banks))                                        # uniform fill of a (range, bank) bucket
        assert lay["cap"] >= 1.5 * mean, (n, lay, mean)
        need = header + plan + a256(8 * lay["ovf_slots"]) + a256(8 * ranges * banks * lay["cap"]) + a256(4 * G) + a256(16 * ranges)
        assert fwd >= need, (n, fwd, need)
        assert bwd >= fwd, (n, bwd, fwd)


def test_layout_query_refuses_shapes_without_grouped_kernels():
    import pytest
    import ttemb_native as nat
    assert nat.grouping_layout(nat.make_shape([125, 140, 140], [4, 5, 5], [1, 16, 16, 1]), 0)["ovf_slots"] == 0
    with pytest.raises(RuntimeError):
        nat.grouping_layout(nat.make_shape([23, 29, 31], [32, 2, 2], [1, 16, 16, 1]), 1000)
