"""Exact mode, host side (no GPU): the size queries of the exact kernels' domain, and no spills in their code objects.
The queries run in a child process with no device visible, like test_route_table_is_pinned."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-ttdforgnns_amd")

# (p, q, inner ranks): products, papers100M r32, 4.4.8 / 8, 8.4.4 / 32, rank 12 (off the grouped kernels' list), 2 cores,
# 4 cores (the reference scripts' 4-core table, and a small one), then the out-of-domain shapes
SUPPORTED = [([125, 140, 140], [4, 5, 5], [16, 16]), ([500, 560, 400], [8, 4, 4], [32, 32]),
             ([50, 60, 70], [4, 4, 8], [8, 8]), ([50, 60, 70], [8, 4, 4], [32, 32]), ([125, 140, 140], [4, 5, 5], [12, 12]),
             ([1500, 1700], [8, 8], [16]), ([1, 1, 1], [4, 4, 4], [1, 1]), ([50, 60, 60, 60], [2, 4, 4, 4], [16, 16, 16]),
             ([20, 20, 20, 20], [2, 2, 2, 4], [8, 8, 8])]
UNSUPPORTED = [([125, 140, 140], [4, 5, 5], [64, 64]), ([125, 140, 140], [4, 5, 5], [128, 128]),
               ([125, 140, 140], [4, 5, 5], [256, 256]), ([125, 140, 140], [32, 2, 2], [16, 16]),
               ([20, 20, 20, 20], [2, 2, 2, 4], [64, 64, 64])]


def _sizes(cases):
    code = ("import sys, json; sys.path[:0] = [sys.argv[1]]; import torch; "
            "assert torch.cuda.device_count() == 0, 'the device is not hidden'; import ttemb_native as n; "
            "out = []\n"
            "for p, q, r in json.loads(sys.argv[2]):\n"
            "    s = n.make_shape(p, q, r)\n"
            "    out.append([int(n.LIB.ttemb_exact_workspace_bytes(s, k, k)) for k in (0, 1, 409600)]"
            " + [int(n.LIB.ttemb_exact_plan_bytes(s, 409600))] + [n.exact_unsupported_reason(s)])\n"
            "print(json.dumps(out))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code, PKG, json.dumps(cases)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_exact_workspace_covers_the_domain():
    for case, (w0, w1, w, plan, reason) in zip(SUPPORTED, _sizes(SUPPORTED)):
        assert reason is None, (case, reason)
        assert 0 < w0 <= w1 <= w, (case, w0, w1, w)
        assert plan == 0, case   # the exact kernels keep no plan


def test_exact_rejects_what_it_does_not_cover():
    for case, (w0, w1, w, plan, reason) in zip(UNSUPPORTED, _sizes(UNSUPPORTED)):
        assert w0 == w1 == w == plan == -3, (case, w0, w1, w, plan)   # TTEMB_E_UNSUPPORTED
        assert reason and "exact mode" in reason, (case, reason)


def test_exact_symbols_and_abi():
    code = ("import sys; sys.path[:0] = [sys.argv[1]]; import ttemb_native as n; "
            "assert n.LIB.ttemb_abi_version() == 4; "
            "[getattr(n.LIB, s) for s in n.EXPORTED_SYMBOLS]; "
            "assert n.LIB.ttemb_set_exact_grid(7) == 0 and n.LIB.ttemb_set_exact_grid(0) == 0; "
            "assert n.LIB.ttemb_set_exact_grid(-1) == -1")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code, PKG], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_exact_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "--fail-on-scratch"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "exact_chunk_kernel" in r.stdout or "exact" in r.stdout, "the exact kernels are not in the library"
