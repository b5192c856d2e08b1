"""Max bags, host side (no GPU): the new symbols, the workspace size query, the per-call mode checks, and no spills in the max
kernels.  Queries run in a child process with no device visible, like test_weighted_host.py."""
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


def test_max_symbols_are_exported_and_bound():
    _child("import ttemb_native as n\n"
           "names = ('ttemb_bag_max_workspace_bytes', 'ttemb_bag_max', 'ttemb_bag_max_backward')\n"
           "assert all(s in n.EXPORTED_SYMBOLS for s in names)\n"
           "[getattr(n.LIB, s) for s in names]\n"
           "assert n.LIB.ttemb_bag_max.argtypes is not None and len(n.LIB.ttemb_bag_max.argtypes) == 12\n"
           "assert len(n.LIB.ttemb_bag_max_backward.argtypes) == 8\n"
           "assert callable(n.bag_max) and callable(n.bag_max_backward)\n"
           "assert n.LIB.ttemb_abi_version() == 4")


def test_max_workspace_query():
    _child("import ttemb_native as n\n"
           "f = n.LIB.ttemb_bag_max_workspace_bytes\n"
           "for nnz, B, D in ((0, 0, 4), (1, 1, 4), (409600, 409600, 100), (409600, 1, 100), (5, 0, 1024)):\n"
           "    assert f(nnz, B, D) >= 0, (nnz, B, D)\n"
           "assert f(409600, 1, 100) >= f(512, 1, 100) >= f(0, 1, 100)\n"
           "for nnz, B, D in ((1, 1, 6), (1, 1, 0), (1, 1, -4), (-1, 1, 4), (1, -1, 4)):\n"
           "    assert f(nnz, B, D) == -1, (nnz, B, D)   # TTEMB_E_BADARG\n"
           "assert n.bag_max_workspace_bytes(409600, 1, 100) == f(409600, 1, 100)\n")


def test_per_call_mode_is_checked_before_anything_is_launched():
    # CPU tensors: a call that got past the checks would raise RuntimeError ("no CPU fallback"), not ValueError
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag, TableBatchedTTEmbeddingBag\n"
           "import pytest, torch\n"
           "one = TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], use_cache=False)\n"
           "two = TableBatchedTTEmbeddingBag(2, 1000, 16, [4, 4], [10, 10, 10], [2, 2, 4])\n"
           "idx, offs, w = torch.arange(4), torch.tensor([0, 2, 4]), torch.ones(4)\n"
           "for e in (one, two):\n"
           "    for mode in ('bogus', 'MAX', ''):\n"
           "        with pytest.raises(ValueError):\n"
           "            e(idx, offs, mode=mode)\n"
           "        with pytest.raises(ValueError):\n"
           "            e(idx.view(2, 2), mode=mode)\n"
           "    with pytest.raises(ValueError, match='per_sample_weights'):\n"
           "        e(idx, offs, per_sample_weights=w, mode='max')\n"
           "    for mode in ('max', 'sum', 'mean'):\n"
           "        with pytest.raises(RuntimeError, match='no CPU fallback'):\n"
           "            e(idx, offs, mode=mode)\n"
           "    assert e.mode == 'sum'\n"
           "with pytest.raises(TypeError):\n"
           "    one(idx, offs, True, None, 'max')   # keyword-only\n"
           "for cls, head in ((TTEmbeddingBag, ()), (TableBatchedTTEmbeddingBag, (2,))):\n"
           "    with pytest.raises(ValueError):\n"
           "        cls(*head, 1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], mode='max')   # the constructor still refuses it\n")


def test_max_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "bag_max", "--fail-on-scratch"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("bag_max_partial_kernel", "bag_max_kernel", "bag_max_backward_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
