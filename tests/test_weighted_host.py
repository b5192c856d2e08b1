"""Weighted and mean bags, host side (no GPU): the new symbols, the workspace size query, the constructor's mode check, and
no spills in the bag kernels.  Queries run in a child process with no device visible, like test_exact_host.py."""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-ttdforgnns_amd")


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [sys.argv[1]]\n" + code, PKG], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_bag_symbols_are_exported():
    _child("import ttemb_native as n\n"
           "names = ('ttemb_bag_workspace_bytes', 'ttemb_bag_reduce', 'ttemb_bag_reduce_backward', 'ttemb_bag_mean')\n"
           "assert all(s in n.EXPORTED_SYMBOLS for s in names)\n"
           "[getattr(n.LIB, s) for s in names]\n"
           "assert n.LIB.ttemb_abi_version() == 4")


def test_bag_workspace_query():
    _child("import ttemb_native as n\n"
           "f = n.LIB.ttemb_bag_workspace_bytes\n"
           "for nnz, B, D in ((0, 0, 4), (1, 1, 4), (409600, 409600, 100), (409600, 1, 100), (5, 0, 1024)):\n"
           "    assert f(nnz, B, D) >= 0, (nnz, B, D)\n"
           "assert f(409600, 1, 100) >= f(512, 1, 100) >= f(0, 1, 100)\n"
           "for nnz, B, D in ((1, 1, 6), (1, 1, 0), (1, 1, -4), (-1, 1, 4), (1, -1, 4)):\n"
           "    assert f(nnz, B, D) == -1, (nnz, B, D)   # TTEMB_E_BADARG\n")


def test_mode_is_checked_at_construction():
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag, TableBatchedTTEmbeddingBag\n"
           "import pytest\n"
           "for mode in ('max', 'SUM', ''):\n"
           "    with pytest.raises(ValueError):\n"
           "        TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], use_cache=False, mode=mode)\n"
           "    with pytest.raises(ValueError):\n"
           "        TableBatchedTTEmbeddingBag(2, 1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], mode=mode)\n"
           "e = TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], use_cache=False, mode='mean')\n"
           "assert e.mode == 'mean' and 'mode' not in e.state_dict()\n"
           "assert TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], use_cache=False).mode == 'sum'")


def test_bag_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "bag_", "--fail-on-scratch"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("bag_partial_kernel", "bag_reduce_kernel", "bag_reduce_backward_kernel", "bag_mean_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
